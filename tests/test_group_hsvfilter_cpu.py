"""CPU companion of tests/test_gpu_group_hsvfilter.py: the surfaces the hsvfilter queue of the video group adds (library exports,
header, bindings, documents, the GStreamer shim) and the builder of its launch sets (mi355_selftest_hsvfilter_set_plan: host only,
no device - the function the queue launches from). Addresses are synthetic numbers; nothing is dereferenced."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_hsvfilter_rendezvous", "mi355_group_submit_hsvfilter", "mi355_group_wait_hsvfilter", "mi355_group_hsvfilter_stats",
             "mi355_selftest_hsvfilter_set_plan"]

IDENT = (0.0, 1.0, 0.0, 1.0, 0.0)
VECTOR, LITERAL = 1, 2
BASE = 0x7f0000001000          # 16-byte aligned


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _plan(frames, n_cu=256):
    import mi355fx
    rc, n_sets, out = mi355fx.selftest_hsvfilter_set_plan(frames, n_cu)
    assert rc == 0, rc
    return n_sets, out


def _one(addr, w, h, stride, fmt, st=IDENT, force_generic=0):
    n_sets, out = _plan([(addr, w, h, stride, fmt, st, force_generic)])
    assert n_sets == 1 and out[0]["set"] == 0
    return out[0]


def _hue(h, sv=(1.0, 0.0, 1.0, 0.0)):
    return (float(h),) + tuple(sv)


def test_library_exports_the_new_names():
    lib = C.CDLL(os.path.join(ROOT, "gst-plugins-rs_amd", "libmi355fx.so"))
    for name in NEW_NAMES:
        assert hasattr(lib, name), name


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert re.search(r"#define MI355_HSVFILTER_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)


def test_bindings_documents_and_shim_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("set_hsvfilter_rendezvous", "submit_hsvfilter", "wait_hsvfilter", "hsvfilter_stats"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^HSVFILTER_SET_MAX = 32\b", py, flags=re.M)
    assert "MI355_GROUP_MEMBERS" in doc[doc.index("mi355_group_submit_hsvfilter"):]
    shim = _read("gst", "gsthsvfilter.c")
    for call in ("mi355_group_shared(", "mi355_group_set_hsvfilter_rendezvous(", "mi355_group_submit_hsvfilter(", "mi355_group_wait_hsvfilter(", "MI355_GROUP_MEMBERS"):
        assert call in shim, call


def test_python_classes_carry_the_methods():
    import mi355fx
    for method in ("set_hsvfilter_rendezvous", "submit_hsvfilter", "wait_hsvfilter", "hsvfilter_stats"):
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.selftest_hsvfilter_set_plan)
    assert mi355fx.HSVFILTER_SET_MAX == 32
    assert C.sizeof(mi355fx.HsvFilterPlanFrame) == 48 and C.sizeof(mi355fx.HsvFilterPlanOut) == 32


def test_classes_by_geometry():
    o = _one(BASE, 8, 2, 32, "RGBx")
    assert (o["launch"], o["units"], o["blocks"], o["first_block"]) == (VECTOR, 4, 1, 0)
    o = _one(BASE + 4, 8, 2, 32, "RGBx")                              # the same frame off the 16-byte grid
    assert (o["launch"], o["units"]) == (LITERAL, 16)
    o = _one(BASE + 4, 4, 1, 12, "RGB")                               # 3-byte: a 4-byte aligned base is enough
    assert (o["launch"], o["units"]) == (VECTOR, 1)
    assert _one(BASE + 2, 4, 1, 12, "RGB")["launch"] == LITERAL
    o = _one(BASE, 5, 1, 15, "RGB")                                   # 15 bytes: no whole group of 12
    assert (o["launch"], o["units"]) == (LITERAL, 5)
    assert _one(BASE, 3, 1, 12, "BGRx")["launch"] == LITERAL          # 12 bytes: no whole group of 16 (packed: not the rowpad class)
    # padded rows: the header's promise - the vector launch for a 4-byte format with base and stride on 16-byte multiples
    # (ceil(width / 4) groups per row), the literal launch for every other padded row
    o = _one(BASE, 8, 2, 48, "RGBx")
    assert (o["launch"], o["units"]) == (VECTOR, 4)
    o = _one(BASE, 5, 3, 32, "xBGR")
    assert (o["launch"], o["units"]) == (VECTOR, 6)
    o = _one(BASE, 8, 2, 40, "RGBx")
    assert (o["launch"], o["units"]) == (LITERAL, 16)
    assert _one(BASE + 4, 8, 2, 48, "RGBx")["launch"] == LITERAL
    assert _one(BASE, 8, 2, 48, "RGB")["launch"] == LITERAL
    for w, h in ((0, 2), (8, 0), (0, 0)):
        o = _one(BASE, w, h, 32, "RGBx")
        assert (o["launch"], o["blocks"], o["units"], o["variant"]) == (0, 0, 0, -1)
    # every one of the ten formats has both classes
    import mi355fx
    for fmt, (ps, _, _) in mi355fx.FMT_LAYOUT.items():
        assert _one(BASE, 16, 3, 16 * ps, fmt)["launch"] == VECTOR, fmt
        assert _one(BASE + 1, 16, 3, 16 * ps, fmt)["launch"] == LITERAL, fmt


def test_variants():
    f32 = np.float32
    v = lambda hue, sv=(1.0, 0.0, 1.0, 0.0), fg=0: _one(BASE, 8, 2, 32, "RGBx", _hue(hue, sv), fg)
    above360, above_wide = float(np.nextafter(f32(360.0), f32(np.inf))), float(np.nextafter(f32(4194304.0), f32(np.inf)))
    assert above360 > 360.0 and above_wide > 4194304.0
    # narrow classes: bits 0-1 zero / positive / negative, bit 2 identity saturation and value
    assert [v(h)["variant"] for h in (0.0, 90.0, -90.0, 360.0, -360.0)] == [4, 5, 6, 5, 6]
    # wide classes: bit 3, the sign in bit 0
    assert [v(h)["variant"] for h in (above360, -above360, 4194304.0, -4194304.0)] == [12, 13, 12, 13]
    assert all(v(h)["launch"] == VECTOR for h in (0.0, 90.0, -90.0, 360.0, -360.0, above360, 4194304.0, -4194304.0))
    # what only the literal arithmetic computes
    for h in (above_wide, -above_wide, 5e-31, -5e-31, float("nan"), float("inf"), float("-inf")):
        o = v(h)
        assert (o["launch"], o["variant"], o["units"]) == (LITERAL, -1, 16), h
    # identity against non-identity saturation / value: bit 2
    for sv in ((1.5, 0.0, 1.0, 0.0), (1.0, 0.1, 1.0, 0.0), (1.0, 0.0, 0.5, 0.0), (1.0, 0.0, 1.0, -0.1)):
        for h in (0.0, 90.0, -90.0, above360, -4194304.0):
            assert v(h, sv)["variant"] == v(h)["variant"] & ~4 and v(h)["variant"] & 4, (h, sv)
    # FORCE_GENERIC
    o = v(90.0, fg=1)
    assert (o["launch"], o["variant"]) == (LITERAL, -1)
    # in the literal launch a narrow shift keeps the single-pixel FAST routine, a wide one has none
    assert _one(BASE + 4, 8, 2, 32, "RGBx", _hue(90.0))["variant"] == 5
    assert _one(BASE + 4, 8, 2, 32, "RGBx", _hue(400.0))["variant"] == -1


def test_sets():
    fr = lambda addr, w=8, h=2, stride=32: (addr, w, h, stride, "RGBx", IDENT)
    n_sets, out = _plan([fr(BASE + 64 * k) for k in range(33)])       # 33 disjoint frames, back to back
    assert n_sets == 2 and [o["set"] for o in out] == [0] * 32 + [1]
    assert out[32]["first_block"] == 0                                # a set's launches begin at block 0
    n_sets, out = _plan([fr(BASE), fr(BASE)])                         # the same bytes twice
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    n_sets, out = _plan([fr(BASE, 64, 8, 256), fr(BASE + 256 + 16, 4, 2, 256)])   # a sub-rectangle of the first
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    n_sets, out = _plan([fr(BASE + 256 + 16, 4, 2, 256), fr(BASE, 64, 8, 256)])   # ... in the other order
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    n_sets, out = _plan([fr(BASE), fr(BASE + 64)])                    # back to back in one allocation
    assert n_sets == 1 and [o["set"] for o in out] == [0, 0]
    n_sets, out = _plan([fr(BASE), fr(BASE + 63, 1, 1, 4)])           # the last byte of the first
    assert n_sets == 2
    # two padded frames side by side in one picture: their rows interleave, their RANGES meet - conservative, a new set
    n_sets, out = _plan([fr(BASE, 4, 4, 64), fr(BASE + 32, 4, 4, 64)])
    assert n_sets == 2
    n_sets, out = _plan([fr(BASE), fr(BASE + 4096), fr(BASE + 16, 4, 1, 16)])     # A, B, A' with A' inside A
    assert n_sets == 2 and [o["set"] for o in out] == [0, 0, 1]
    n_sets, out = _plan([fr(BASE), fr(BASE, 0, 2, 32), fr(BASE, 8, 0, 32), fr(BASE + 64)])   # a frame without a pixel has no byte
    assert n_sets == 1 and [o["launch"] for o in out] == [VECTOR, 0, 0, VECTOR]
    assert _plan([]) == (0, [])


def test_blocks():
    hd = lambda addr: (addr, 1920, 1080, 7680, "BGRx", IDENT)
    step = 1920 * 1080 * 4
    # the figures of test_plan_values in the hsvdetect file: 32 packed 1080p frames share 256 x 64 blocks, four get the lone grid each
    n_sets, out = _plan([hd(BASE + k * step) for k in range(32)])
    assert n_sets == 1 and [o["blocks"] for o in out] == [512] * 32 and all(o["units"] == 518400 for o in out)
    assert [o["first_block"] for o in out] == [512 * k for k in range(32)]
    n_sets, out = _plan([hd(BASE + k * step) for k in range(4)])
    assert [o["blocks"] for o in out] == [1013] * 4
    # first_block is the running sum PER LAUNCH: vector and literal frames interleaved
    frames, addr = [], BASE
    for k in range(12):
        w = 64 + 32 * k
        literal = k % 3 == 1
        frames.append((addr + (4 if literal else 0), w, 16, w * 4, "RGBA", _hue(30.0 * k)))
        addr += (w * 4 * 16 + 4 + 15) // 16 * 16
    n_sets, out = _plan(frames, n_cu=8)
    assert n_sets == 1
    for launch, per_block in ((VECTOR, 512), (LITERAL, 256)):
        running = 0
        for o in out:
            if o["launch"] != launch:
                continue
            assert o["first_block"] == running and o["blocks"] == -(-o["units"] // per_block)
            running += o["blocks"]
        assert running > 0
    # a squeezed plan: equal frames get equal shares, every frame at least a block, the total within the budget
    n_sets, out = _plan([hd(BASE + k * step) for k in range(32)], n_cu=1)
    assert [o["blocks"] for o in out] == [2] * 32
    n_sets, out = _plan([hd(BASE)] + [(BASE + step + 64 * k, 4, 3, 16, "RGBx", IDENT) for k in range(31)], n_cu=1)
    assert [o["blocks"] for o in out] == [33] + [1] * 31


def test_refusals():
    import mi355fx
    S = mi355fx.selftest_hsvfilter_set_plan
    ok = (BASE, 8, 2, 32, "RGBx", IDENT)
    assert S([ok])[0] == 0
    assert S([ok], n_cu=0)[0] != 0 and S([ok], n_cu=-1)[0] != 0
    assert S(None)[0] != 0                                            # null arrays with a frame
    L = mi355fx.load_library()
    fr, out = (mi355fx.HsvFilterPlanFrame * 1)(), (mi355fx.HsvFilterPlanOut * 1)()
    fr[0] = mi355fx.HsvFilterPlanFrame(BASE, 8, 2, 32, 0, mi355fx.HsvSettings(*IDENT), 0)
    n = C.c_int(0)
    assert L.mi355_selftest_hsvfilter_set_plan(256, fr, 1, out, C.byref(n)) == 0 and n.value == 1
    assert L.mi355_selftest_hsvfilter_set_plan(256, fr, 1, out, None) != 0
    assert L.mi355_selftest_hsvfilter_set_plan(256, fr, 1, None, C.byref(n)) != 0
    assert L.mi355_selftest_hsvfilter_set_plan(256, fr, -1, out, C.byref(n)) != 0
    assert L.mi355_selftest_hsvfilter_set_plan(256, None, 0, None, C.byref(n)) == 0 and n.value == 0
    # frames a submit refuses
    assert S([(BASE, 8, 2, 32, "RGBA64_LE", IDENT)])[0] != 0
    assert S([(BASE, 8, 2, 32, 12, IDENT)])[0] != 0
    assert S([(BASE, 8, 2, 31, "RGBx", IDENT)])[0] != 0               # stride below the line bytes
    assert S([(BASE, -1, 2, 32, "RGBx", IDENT)])[0] != 0
    assert S([(BASE, 8, -1, 32, "RGBx", IDENT)])[0] != 0
    assert S([(0, 8, 2, 32, "RGBx", IDENT)])[0] != 0                  # a null frame with a pixel
    assert S([(0, 0, 2, 0, "RGBx", IDENT)])[0] == 0                   # ... and without one
