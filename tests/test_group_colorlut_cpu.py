"""CPU companion of tests/test_gpu_group_colorlut.py: the surfaces the colorlut queue of the video group adds (library exports,
header, bindings, documents, the GStreamer shim) and the builder of its launch sets (mi355_selftest_colorlut_set_plan: host only,
no device - the function the queue launches from). Addresses are synthetic numbers; nothing is dereferenced."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_colorlut_rendezvous", "mi355_group_submit_colorlut", "mi355_group_wait_colorlut", "mi355_group_colorlut_stats",
             "mi355_selftest_colorlut_set_plan"]

VECTOR, LITERAL = 1, 2
FLAT, ROWPAD = 1, 2
SRC = 0x7f0000001000           # 16-byte aligned
DST = 0x7f0080001000
VEC_GRID, LIT_GRID = (512, 16), (256, 8)      # (units per block, blocks per CU) of the two launches


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _plan(frames, n_cu=256):
    import mi355fx
    rc, n_sets, out = mi355fx.selftest_colorlut_set_plan(frames, n_cu)
    assert rc == 0, rc
    return n_sets, out


def _fr(src, dst, w, h, fmt="RGBA", src_stride=None, dst_stride=None, force_generic=0):
    bpp = 4 if fmt == "RGBA" else 8
    return (src, w * bpp if src_stride is None else src_stride, dst, w * bpp if dst_stride is None else dst_stride, w, h, fmt, force_generic)


def _one(*a, **k):
    n_sets, out = _plan([_fr(*a, **k)])
    assert n_sets == 1 and out[0]["set"] == 0
    return out[0]


def hsvdetect_plan(n_cu, per_cu, per_block, units):
    """mi355_selftest_hsvdetect_plan's rule, restated: every job its want if the wants fit n_cu * per_cu blocks, else one block each
    and the rest of the budget in proportion to what the jobs still want, rounded down."""
    want = [-(-u // per_block) for u in units]
    budget = n_cu * per_cu
    if sum(want) <= budget:
        blocks = want
    else:
        with_units = sum(1 for w in want if w)
        still = sum(w - 1 for w in want if w)
        spare = max(budget - with_units, 0)
        blocks = [1 + (w - 1) * spare // max(still, 1) if w else 0 for w in want]
    first, nxt = [], 0
    for b in blocks:
        first.append(nxt)
        nxt += b
    return first, blocks


def test_library_exports_the_new_names():
    lib = C.CDLL(os.path.join(ROOT, "gst-plugins-rs_amd", "libmi355fx.so"))
    for name in NEW_NAMES:
        assert hasattr(lib, name), name


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert re.search(r"#define MI355_COLORLUT_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)
    # the borrowing rule is said where the entry is declared
    block = h[h.index("colorlut frames of INDEPENDENT"):h.index("#define MI355_COLORLUT_SET_MAX")]
    for word in ("borrowed", "mi355_colorlut_load", "mi355_colorlut_unload", "mi355_ctx_destroy"):
        assert word in block, word


def test_bindings_documents_and_shim_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    design = _read("DESIGN.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("set_colorlut_rendezvous", "submit_colorlut", "wait_colorlut", "colorlut_stats"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^COLORLUT_SET_MAX = 32\b", py, flags=re.M)
    assert "MI355_GROUP_MEMBERS" in doc[doc.index("mi355_group_submit_colorlut"):]
    assert "4.7.2" in design and "colorlut_jobs_kernel" in design and "colorlut_rows_jobs_kernel" in design
    assert "mi355_group_submit_colorlut" in _read("README.md")
    shim = _read("gst", "gstcolorlut.c")
    for call in ("mi355_group_shared(", "mi355_group_release(", "mi355_group_set_colorlut_rendezvous(", "mi355_group_submit_colorlut(", "mi355_group_wait_colorlut(",
                 "MI355_GROUP_MEMBERS", "mi355_colorlut_frames_device("):
        assert call in shim, call
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_colorlut_group.py"))


def test_python_classes_carry_the_methods():
    import mi355fx
    for method in ("set_colorlut_rendezvous", "submit_colorlut", "wait_colorlut", "colorlut_stats"):
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.selftest_colorlut_set_plan)
    assert mi355fx.COLORLUT_SET_MAX == 32
    assert C.sizeof(mi355fx.ColorLutPlanFrame) == 40 and C.sizeof(mi355fx.ColorLutPlanOut) == 32


def test_classes_by_geometry():
    # flat: both sides packed, both bases and the byte count multiples of 16
    o = _one(SRC, DST, 8, 2)
    assert (o["launch"], o["geometry"], o["units"], o["blocks"], o["first_block"]) == (VECTOR, FLAT, 4, 1, 0)
    o = _one(SRC, DST, 3, 4)                                          # 48 bytes in rows of 12: packed, whole groups
    assert (o["launch"], o["geometry"], o["units"]) == (VECTOR, FLAT, 3)
    # a base off by 4, on either side: literal
    for s, d in ((SRC + 4, DST), (SRC, DST + 4), (SRC + 4, DST + 4)):
        o = _one(s, d, 8, 2)
        assert (o["launch"], o["geometry"], o["units"]) == (LITERAL, 0, 16), (s, d)
    # a byte count off by 4 at packed rows: no whole groups and no 16-byte strides - literal
    for w, h in ((5, 1), (3, 1), (5, 3), (7, 1)):
        o = _one(SRC, DST, w, h)
        assert (o["launch"], o["units"]) == (LITERAL, w * h), (w, h)
    # rowpad: a padded side, bases and both strides multiples of 16; ceil(width / 4) groups per row
    o = _one(SRC, DST, 5, 3, src_stride=32, dst_stride=32)
    assert (o["launch"], o["geometry"], o["units"]) == (VECTOR, ROWPAD, 6)
    o = _one(SRC, DST, 8, 2, src_stride=48)                           # one side padded, the other packed (32)
    assert (o["launch"], o["geometry"], o["units"]) == (VECTOR, ROWPAD, 4)
    o = _one(SRC, DST, 8, 2, dst_stride=64)
    assert (o["launch"], o["geometry"], o["units"]) == (VECTOR, ROWPAD, 4)
    o = _one(SRC, DST, 5, 1, src_stride=32, dst_stride=32)            # one row of 20 bytes in 32: rowpad where packed it was literal
    assert (o["launch"], o["geometry"], o["units"]) == (VECTOR, ROWPAD, 2)
    # a stride off by 4, on either side: literal
    for ss, ds in ((36, 32), (32, 36), (36, 36), (48, 44)):
        o = _one(SRC, DST, 8, 2, src_stride=ss, dst_stride=ds)
        assert (o["launch"], o["geometry"], o["units"]) == (LITERAL, 0, 16), (ss, ds)
    assert _one(SRC + 4, DST, 8, 2, src_stride=48, dst_stride=48)["launch"] == LITERAL
    assert _one(SRC, DST + 8, 8, 2, src_stride=48, dst_stride=48)["launch"] == LITERAL
    # RGBA64: always literal, aligned and packed or not
    for fmt in ("RGBA64_LE", "RGBA64_BE"):
        o = _one(SRC, DST, 8, 2, fmt)
        assert (o["launch"], o["geometry"], o["units"]) == (LITERAL, 0, 16), fmt
        assert _one(SRC, DST, 8, 2, fmt, src_stride=80, dst_stride=96)["launch"] == LITERAL
        assert _one(SRC + 2, DST, 3, 2, fmt)["launch"] == LITERAL
    # the force-generic field
    o = _one(SRC, DST, 8, 2, force_generic=1)
    assert (o["launch"], o["geometry"], o["units"]) == (LITERAL, 0, 16)
    assert _one(SRC, DST, 5, 3, src_stride=32, dst_stride=32, force_generic=1)["launch"] == LITERAL
    # no pixel: no job
    for w, h in ((0, 2), (8, 0), (0, 0)):
        o = _one(SRC, DST, w, h, src_stride=32, dst_stride=32)
        assert (o["launch"], o["geometry"], o["blocks"], o["units"]) == (0, 0, 0, 0)


def test_units_and_blocks_follow_hsvdetect_plan():
    step = 1920 * 1080 * 4
    hd = lambda k, **kw: _fr(SRC + k * step, DST + k * step, 1920, 1080, **kw)
    for n, n_cu in ((32, 256), (4, 256), (32, 1), (3, 7)):
        n_sets, out = _plan([hd(k) for k in range(n)], n_cu=n_cu)
        assert n_sets == 1 and all(o["launch"] == VECTOR and o["units"] == 518400 for o in out)
        first, blocks = hsvdetect_plan(n_cu, VEC_GRID[1], VEC_GRID[0], [518400] * n)
        assert [o["first_block"] for o in out] == first and [o["blocks"] for o in out] == blocks, (n, n_cu)
    n_sets, out = _plan([hd(k) for k in range(32)])
    assert [o["blocks"] for o in out] == [128] * 32                   # 256 CUs x 16 blocks shared by 32 equal frames
    n_sets, out = _plan([hd(k) for k in range(2)])
    assert [o["blocks"] for o in out] == [1013] * 2                   # the wants fit: 518400 / 512, rounded up
    # the literal launch: pixels, 256 per block, 8 blocks per CU
    for n, n_cu in ((32, 256), (2, 256), (5, 3)):
        n_sets, out = _plan([hd(k, fmt="RGBA", force_generic=1) for k in range(n)], n_cu=n_cu)
        assert all(o["launch"] == LITERAL and o["units"] == 1920 * 1080 for o in out)
        first, blocks = hsvdetect_plan(n_cu, LIT_GRID[1], LIT_GRID[0], [1920 * 1080] * n)
        assert [o["first_block"] for o in out] == first and [o["blocks"] for o in out] == blocks, (n, n_cu)
    # first_block is the running sum PER LAUNCH: vector and literal frames interleaved, unequal sizes, a squeezed budget
    frames, at = [], 0
    for k in range(12):
        w = 64 + 32 * k
        lit = k % 3 == 1
        frames.append(_fr(SRC + at + (4 if lit else 0), DST + at + (4 if lit else 0), w, 16))
        at += (w * 4 * 16 + 4 + 15) // 16 * 16
    for n_cu in (8, 1):
        n_sets, out = _plan(frames, n_cu=n_cu)
        assert n_sets == 1
        for launch, (per_block, per_cu) in ((VECTOR, VEC_GRID), (LITERAL, LIT_GRID)):
            mine = [o for o in out if o["launch"] == launch]
            first, blocks = hsvdetect_plan(n_cu, per_cu, per_block, [o["units"] for o in mine])
            assert [o["first_block"] for o in mine] == first and [o["blocks"] for o in mine] == blocks and sum(blocks) > 0
            assert all(b >= 1 for b in blocks)
    # a big frame among small ones takes what they leave
    n_sets, out = _plan([hd(0)] + [_fr(SRC + step + 64 * k, DST + step + 64 * k, 4, 3) for k in range(31)], n_cu=1)
    assert [o["blocks"] for o in out] == hsvdetect_plan(1, VEC_GRID[1], VEC_GRID[0], [518400] + [3] * 31)[1]


def test_sets():
    fr = lambda s, d, w=8, h=2, **kw: _fr(s, d, w, h, **kw)
    n_sets, out = _plan([fr(SRC + 64 * k, DST + 64 * k) for k in range(33)])      # 33 disjoint frames, back to back
    assert n_sets == 2 and [o["set"] for o in out] == [0] * 32 + [1]
    assert out[32]["first_block"] == 0                                            # a set's launches begin at block 0
    n_sets, out = _plan([fr(SRC + 64 * k, DST + 64 * k) for k in range(65)])
    assert n_sets == 3 and [o["set"] for o in out] == [0] * 32 + [1] * 32 + [2]
    # frames that share a SOURCE share a set
    n_sets, out = _plan([fr(SRC, DST), fr(SRC, DST + 64), fr(SRC + 16, DST + 128, 4, 1)])
    assert n_sets == 1
    # the three cross-frame overlaps, each closing the set in front of the later frame
    n_sets, out = _plan([fr(SRC, DST), fr(DST, DST + 4096)])                      # B's source is A's destination
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    n_sets, out = _plan([fr(SRC, DST), fr(SRC + 4096, DST)])                      # B's destination meets A's destination
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    n_sets, out = _plan([fr(SRC, DST), fr(SRC + 4096, SRC)])                      # B's destination meets A's source
    assert n_sets == 2 and [o["set"] for o in out] == [0, 1]
    # by one byte, and not by none
    n_sets, out = _plan([fr(SRC, DST), fr(SRC + 4096, DST + 63, 1, 1)])
    assert n_sets == 2
    n_sets, out = _plan([fr(SRC, DST), fr(SRC + 4096, DST + 64, 1, 1)])
    assert n_sets == 1
    n_sets, out = _plan([fr(SRC, DST), fr(DST + 60, DST + 4096, 1, 1)])           # reads the last pixel A writes
    assert n_sets == 2
    # a frame in the middle of the set is seen too, and the set after the break starts over
    n_sets, out = _plan([fr(SRC, DST), fr(SRC + 64, DST + 64), fr(DST + 64, DST + 4096), fr(SRC + 128, DST + 128)])
    assert n_sets == 2 and [o["set"] for o in out] == [0, 0, 1, 1]
    # two sub-pictures side by side in one padded destination picture: their rows interleave, their RANGES meet - conservative
    n_sets, out = _plan([fr(SRC, DST, 4, 4, dst_stride=64), fr(SRC + 64, DST + 32, 4, 4, dst_stride=64)])
    assert n_sets == 2
    # ... and side by side in one SOURCE picture, written to separate places: readers only, one set
    n_sets, out = _plan([fr(SRC, DST, 4, 4, src_stride=64), fr(SRC + 32, DST + 4096, 4, 4, src_stride=64)])
    assert n_sets == 1
    # a frame without a pixel has no byte
    n_sets, out = _plan([fr(SRC, DST), fr(SRC, DST, 0, 2), fr(DST, SRC, 8, 0), fr(SRC + 64, DST + 64)])
    assert n_sets == 1 and [o["launch"] for o in out] == [VECTOR, 0, 0, VECTOR]
    assert _plan([]) == (0, [])


def test_refusals():
    import mi355fx
    S = mi355fx.selftest_colorlut_set_plan
    ok = _fr(SRC, DST, 8, 2)
    assert S([ok])[0] == 0
    assert S([ok], n_cu=0)[0] != 0 and S([ok], n_cu=-1)[0] != 0
    assert S(None)[0] != 0                                            # null arrays with a frame
    L = mi355fx.load_library()
    fr, out = (mi355fx.ColorLutPlanFrame * 1)(), (mi355fx.ColorLutPlanOut * 1)()
    fr[0] = mi355fx.ColorLutPlanFrame(SRC, DST, 32, 32, 8, 2, mi355fx.FMT["RGBA"], 0)
    n = C.c_int(0)
    assert L.mi355_selftest_colorlut_set_plan(256, fr, 1, out, C.byref(n)) == 0 and n.value == 1
    assert L.mi355_selftest_colorlut_set_plan(256, fr, 1, out, None) != 0
    assert L.mi355_selftest_colorlut_set_plan(256, fr, 1, None, C.byref(n)) != 0
    assert L.mi355_selftest_colorlut_set_plan(256, fr, -1, out, C.byref(n)) != 0
    assert L.mi355_selftest_colorlut_set_plan(256, None, 0, None, C.byref(n)) == 0 and n.value == 0
    # frames a submit refuses
    for fmt in ("RGBx", "BGRA", "RGB", 12, -1):                        # not one of the three formats
        assert S([_fr(SRC, DST, 8, 2, fmt)])[0] != 0, fmt
    assert S([_fr(SRC, DST, -1, 2, src_stride=32, dst_stride=32)])[0] != 0      # negative sizes
    assert S([_fr(SRC, DST, 8, -1)])[0] != 0
    assert S([_fr(0, DST, 8, 2)])[0] != 0                             # a null side with a pixel
    assert S([_fr(SRC, 0, 8, 2)])[0] != 0
    assert S([_fr(0, 0, 0, 2)])[0] == 0                               # ... and without one
    assert S([_fr(SRC, DST, 8, 2, src_stride=31)])[0] != 0            # strides below the row bytes
    assert S([_fr(SRC, DST, 8, 2, dst_stride=31)])[0] != 0
    assert S([_fr(SRC, DST, 8, 2, "RGBA64_LE", src_stride=63)])[0] != 0
    assert S([_fr(SRC, DST, 8, 2, src_stride=-32)])[0] != 0
    # the queue's own: a frame whose own source and destination ranges meet
    assert S([_fr(SRC, SRC, 8, 2)])[0] != 0
    assert S([_fr(SRC, SRC + 63, 8, 2)])[0] != 0                      # by one byte
    assert S([_fr(SRC + 63, SRC, 8, 2)])[0] != 0
    assert S([_fr(SRC, SRC + 64, 8, 2)])[0] == 0                      # back to back
    assert S([_fr(SRC, SRC + 32, 4, 4, src_stride=64, dst_stride=64)])[0] != 0   # side by side in one picture: ranges
    assert S([_fr(SRC, SRC, 0, 2)])[0] == 0                           # no pixel, no byte
