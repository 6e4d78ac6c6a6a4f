"""CPU companion of tests/test_gpu_group_hsvdetect.py: the surfaces the hsvdetector queue of the video group adds (library exports,
header, bindings, documents, the GStreamer shim) and the block plan of one launch of a set (mi355_selftest_hsvdetect_plan: host
only, no device)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_hsvdetect_rendezvous", "mi355_group_submit_hsvdetect", "mi355_group_wait_hsvdetect", "mi355_group_hsvdetect_stats",
             "mi355_selftest_hsvdetect_plan"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(os.path.join(ROOT, "gst-plugins-rs_amd", "libmi355fx.so"))
    L.mi355_selftest_hsvdetect_plan.restype = C.c_int
    L.mi355_selftest_hsvdetect_plan.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                C.POINTER(C.c_uint32)]
    return L


def _plan(lib, n_cu, per_cu, per_block, units):
    n = len(units)
    first, blocks, total = (C.c_uint32 * n)(), (C.c_uint32 * n)(), C.c_uint32(12345)
    rc = lib.mi355_selftest_hsvdetect_plan(n_cu, per_cu, per_block, n, (C.c_uint64 * n)(*units), first, blocks, C.byref(total))
    return rc, list(first), list(blocks), total.value


def test_library_exports_the_new_names(lib):
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
    lib.mi355_abi_version.restype = C.c_int
    assert lib.mi355_abi_version() == 1


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert re.search(r"#define MI355_HSVDETECT_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)


def test_bindings_documents_and_shim_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("set_hsvdetect_rendezvous", "submit_hsvdetect", "wait_hsvdetect", "hsvdetect_stats", "hsvdetect_frames_device"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^HSVDETECT_SET_MAX = 32\b", py, flags=re.M)
    assert "MI355_GROUP_MEMBERS" in doc[doc.index("mi355_group_submit_hsvdetect"):]
    assert "mi355_group_submit_hsvdetect(" in _read("gst", "gsthsvdetector.c")


def test_python_classes_carry_the_methods():
    import mi355fx
    for method in ("set_hsvdetect_rendezvous", "submit_hsvdetect", "wait_hsvdetect", "hsvdetect_stats"):
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.Context.hsvdetect_frames_device)
    assert mi355fx.HSVDETECT_SET_MAX == 32


UNIT_LISTS = [[0], [1], [0, 5, 0], [512, 513], [129600] * 32, [2**40], [518400] + [12] * 31]


@pytest.mark.parametrize("n_cu", [1, 8, 256])
@pytest.mark.parametrize("per_cu,per_block", [(64, 512), (32, 256)])
@pytest.mark.parametrize("units", UNIT_LISTS, ids=lambda u: "%dx%d" % (len(u), u[0]))
def test_plan_properties(lib, n_cu, per_cu, per_block, units):
    rc, first, blocks, total = _plan(lib, n_cu, per_cu, per_block, units)
    assert rc == 0
    running = 0
    for j, u in enumerate(units):
        assert first[j] == running, (j, first, blocks)
        running += blocks[j]
        if u == 0:
            assert blocks[j] == 0
        else:
            assert 1 <= blocks[j] <= -(-u // per_block), (j, blocks[j])
    assert total == running == sum(blocks)
    assert total <= max(n_cu * per_cu, sum(1 for u in units if u))
    for a in range(len(units)):
        for b in range(a):
            if units[a] == units[b]:
                assert blocks[a] == blocks[b], (a, b, blocks)


def test_plan_values(lib):
    """32 packed 1080p frames share the 256 x 64 blocks equally; four of them get the grid of the lone launch each (the wants fit);
    a big frame among small ones takes what they leave."""
    def blocks(n_cu, per_cu, per_block, units):
        rc, first, b, total = _plan(lib, n_cu, per_cu, per_block, units)
        assert rc == 0
        return b

    assert blocks(256, 64, 512, [518400] * 32) == [512] * 32
    assert blocks(256, 64, 512, [518400] * 4) == [1013] * 4
    assert blocks(256, 64, 512, [512]) == [1] and blocks(256, 64, 512, [513]) == [2]
    # 64 blocks in all, 31 of them taken by the small frames' one each: the big frame has the other 33 of the 1013 it wants
    assert blocks(1, 64, 512, [518400] + [12] * 31) == [33] + [1] * 31
    # fewer blocks than frames: one each
    assert blocks(1, 8, 512, [518400] * 32) == [1] * 32
    # a frame's position in the set does not change its share
    assert blocks(1, 64, 512, [12] * 31 + [518400]) == [1] * 31 + [33]


def test_plan_refusals(lib):
    ok = (256, 64, 512, [5])
    assert _plan(lib, *ok)[0] == 0
    assert _plan(lib, 0, 64, 512, [5])[0] != 0
    assert _plan(lib, 256, 0, 512, [5])[0] != 0
    assert _plan(lib, 256, 64, 0, [5])[0] != 0
    assert _plan(lib, 256, 64, 512, [1] * 33)[0] != 0
    total = C.c_uint32(0)
    one = (C.c_uint32 * 1)()
    units = (C.c_uint64 * 1)(5)
    f = lib.mi355_selftest_hsvdetect_plan
    assert f(256, 64, 512, -1, units, one, one, C.byref(total)) != 0
    assert f(256, 64, 512, 1, None, one, one, C.byref(total)) != 0
    assert f(256, 64, 512, 1, units, None, one, C.byref(total)) != 0
    assert f(256, 64, 512, 1, units, one, None, C.byref(total)) != 0
    assert f(256, 64, 512, 0, None, None, None, C.byref(total)) == 0 and total.value == 0
