"""CPU companion of tests/test_gpu_group_colordetect.py: the surfaces the colordetect queue of the video group adds (library
exports, header, bindings, documents) and the block plan of a launch set (mi355_selftest_colordetect_plan: host only, no device)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_colordetect_rendezvous", "mi355_group_submit_colordetect", "mi355_group_wait_colordetect", "mi355_group_colordetect_stats",
             "mi355_selftest_colordetect_plan"]


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
    assert re.search(r"#define MI355_COLORDETECT_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("set_colordetect_rendezvous", "submit_colordetect", "wait_colordetect", "colordetect_stats"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert "MI355_GROUP_MEMBERS" in doc[doc.index("mi355_group_submit_colordetect"):]
    assert "mi355_group_submit_colordetect(" in _read("gst", "gstcolordetect.c")


SAMPLE_LISTS = [[0], [1], [0, 5, 0], [16384, 16385], [24576] + [300] * 31, [2**32 - 1], [2_073_600] * 32]


@pytest.mark.parametrize("n_cu", [1, 8, 256])
@pytest.mark.parametrize("ns", SAMPLE_LISTS, ids=lambda ns: "%dx%d" % (len(ns), ns[0]))
def test_plan_of_a_launch_set(lib, n_cu, ns):
    n = len(ns)
    first, blocks, per, total = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint64 * n)(), C.c_uint32(12345)
    lib.mi355_selftest_colordetect_plan.restype = C.c_int
    lib.mi355_selftest_colordetect_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_uint32)]
    assert lib.mi355_selftest_colordetect_plan(n_cu, n, (C.c_uint64 * n)(*ns), first, blocks, per, C.byref(total)) == 0
    running = 0
    for j in range(n):
        assert first[j] == running, (j, list(first), list(blocks))
        running += blocks[j]
        if ns[j] == 0:
            assert blocks[j] == 0
            continue
        assert 1 <= blocks[j] <= -(-ns[j] // 16384), (j, blocks[j])
        # every sample falls into exactly one block, and no block is empty
        assert blocks[j] * per[j] >= ns[j] > (blocks[j] - 1) * per[j], (j, blocks[j], per[j])
    assert total.value == running
    assert total.value <= max(n_cu, sum(1 for v in ns if v))


def test_plan_shares_the_device_by_sample_count(lib):
    """What the design rests on: 32 equal 4K frames at quality 10 fill 256 CUs with 8 blocks each; a large frame among small ones
    takes what the small ones leave; arguments out of range are refused."""
    lib.mi355_selftest_colordetect_plan.restype = C.c_int

    def plan(n_cu, ns):
        n = len(ns)
        first, blocks, per, total = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint64 * n)(), C.c_uint32(0)
        rc = lib.mi355_selftest_colordetect_plan(C.c_int(n_cu), C.c_int(n), (C.c_uint64 * n)(*ns), first, blocks, per, C.byref(total))
        return rc, list(blocks), total.value

    assert plan(256, [829440] * 32) == (0, [8] * 32, 256)
    rc, blocks, total = plan(256, [8_294_400] + [300] * 7)
    assert rc == 0 and blocks[1:] == [1] * 7 and blocks[0] >= 240 and total <= 256
    assert plan(256, [24576])[1] == [2] and plan(256, [16384])[1] == [1] and plan(256, [16385])[1] == [2]
    assert plan(0, [1])[0] != 0 and plan(256, [2**32])[0] != 0 and plan(256, [1] * 33)[0] != 0
