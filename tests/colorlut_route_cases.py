"""The cases of the colorlut route table: which kernel serves a launch (Context.colorlut_kernel_name()) and the CRC-32 of the whole
destination buffer, for every combination of entry point, pixel format, LUT, MI355_FLAG_LUT_VARIANT, MI355_FLAG_BRICK_SETS,
MI355_FLAG_FUSED_VARIANT, MI355_FLAG_FORCE_GENERIC and geometry at which the host dispatch of csrc/colorlut_kernels.hip can take
another route. Shared by tools/record_colorlut_routes.py (writes tests/golden/colorlut_routes_parent.json at a parent commit) and
tests/test_gpu_colorlut_routes.py (replays them on the tree under test): both run the cases through run_product / run_auto /
run_group below, in the same order, on one context per LUT, so that whatever a context carries from case to case (tables, the
content watch) is carried the same way in both.

The source of every case is one flat colour: no 256-pixel step misses a brick cache it has warmed, the content watch stays at
level 0, and the route is a function of the inputs. The destination is prefilled with a fixed byte pattern before every launch:
row padding, the gap between frames and the tail of the buffer are part of the CRC. Routes that change with content are covered by
test_gpu_brick.py, test_gpu_shared_brick.py and test_gpu_window.py."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorlut_routes_parent.json")

LUTS = ["1d16", "3d17", "3d33", "3d65", "3d66"]      # 65 = kBrickMaxSize, 66 is above it (and above the three-pass kernel's 64)
ENTRIES = ["RGBA", "RGBA64_LE", "RGBA64_BE", "fused"]  # colorlut_frames_device per format; hsv_colorlut_frames_device (RGBA)
VARIANTS = list(range(10))
BRICK_SETS = [0, 32, 48, 64, 512]
HSV = (-33.3, 1.2, -0.05, 0.9, 0.02)                   # the fused entry's settings (not the identity)
KSTABLE = 8                                            # kStableCalls of colorlut_kernels.hip
BUF_BYTES = 24576                                      # the largest case ends at byte 17680 (+ 4 for the offset source)
PIXEL8 = bytes([200, 90, 30, 0x80])
PIXEL16 = bytes([0xC8, 0xA1, 0x5A, 0x33, 0x1E, 0x77, 0x80, 0x01])

# name: (width, height, frames, bytes the row stride is padded by, rows the frame pitch is longer than stride * height, source offset)
GEOMS = {
    "64x8": (64, 8, 1, 0, 0, 0),            # packed, below the tiled table kernel's 128-pixel floor
    "128x8": (128, 8, 1, 0, 0, 0),          # packed
    "128x8x2": (128, 8, 2, 0, 0, 0),        # two frames back to back
    "pad16x2": (128, 8, 2, 16, 0, 0),       # padded rows, frames stride * height apart: one tall picture
    "pad16x2gap": (128, 8, 2, 16, 1, 0),    # padded rows, frames one row further apart
    "srcoff4": (128, 8, 1, 0, 0, 4),        # source base 4 bytes off a 16-byte boundary
    "126x8": (126, 8, 1, 0, 0, 0),          # width not a multiple of 4
}
PACKED = ["64x8", "128x8"]

# every last_kernel literal of csrc/colorlut_kernels.hip at the recorded commit. The golden must hold each of them at least once, but
# for the two that need launches of megapixels and are asserted by test_gpu_window.py / test_gpu_shared_brick.py.
KERNEL_NAMES = [
    "colorlut3d_brick_kernel<HSV> (64 sets)", "colorlut3d_brick_kernel<HSV> (48 sets)", "colorlut3d_brick_kernel<HSV>", "colorlut3d_lds_kernel<HSV>",
    "colorlut1d_lds_kernel", "colorlut3d_shared_kernel", "colorlut3d_brick_kernel (64 sets)", "colorlut3d_brick_kernel (48 sets)",
    "colorlut3d_brick_kernel", "colorlut3d_lds_kernel", "colorlut3d_brick_kernel<RGBA64> (64 sets)", "colorlut3d_brick_kernel<RGBA64>",
    "colorlut3d_lds64_kernel", "colorlut1d_lds64_kernel", "colorlut_rows_kernel", "colorlut_window_kernel", "colorlut_table_tiled_kernel",
    "colorlut_table_kernel", "colorlut_table_tiled_multi_kernel",
]
NOT_COVERED = ["colorlut_window_kernel", "colorlut3d_shared_kernel"]


def lut_table(name):
    """(is3d, size, float32 table in the layout mi355_colorlut_load takes): the identity plus a small polynomial bend, from integer
    arithmetic and one float32 division per value, so that every machine makes the same bits."""
    size = int(name[2:])
    g = np.arange(size, dtype=np.float32) / np.float32(size - 1)
    bend = (g * (np.float32(1) - g)).astype(np.float32)
    if name.startswith("1d"):
        return False, size, np.concatenate([g + bend * np.float32(0.25), g, g - bend * np.float32(0.25)]).astype(np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")      # cell = x + size * y + size^2 * z, x (red) fastest
    bz, by, bx = np.meshgrid(bend, bend, bend, indexing="ij")
    t = np.zeros((size, size, size, 4), np.float32)
    t[..., 0] = x + by * np.float32(0.125)
    t[..., 1] = y - bz * np.float32(0.125)
    t[..., 2] = z + bx * np.float32(0.0625)
    return True, size, t.reshape(-1)


def product_cases():
    """[(name, entry, variant, brick_sets, fused_variant, force_generic, geometry)] of one LUT, in the order they run: the variant
    changes slowest within an entry, so a context rebuilds its memoised table a few times, not once per case."""
    out = []
    for entry in ENTRIES:
        for fv, fg in ((0, 0), (1, 0), (0, 1)):
            for v in VARIANTS:
                for sets in (BRICK_SETS if (fv, fg) == (0, 0) else [0]):
                    for geom in GEOMS:
                        out.append(("%s/v%d/s%d/fv%d/fg%d/%s" % (entry, v, sets, fv, fg, geom), entry, v, sets, fv, fg, geom))
    return out


def prefill():
    return ((np.arange(BUF_BYTES, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)


def _flat(pixel):
    return np.frombuffer(pixel * (BUF_BYTES // len(pixel)), np.uint8).copy()


class _Buffers:
    def __init__(self, ctx):
        self.ctx = ctx
        self.fill = prefill()
        self.out = np.empty(BUF_BYTES, np.uint8)
        self.src8, self.src16, self.dst = ctx.alloc(BUF_BYTES + 16), ctx.alloc(BUF_BYTES + 16), ctx.alloc(BUF_BYTES)
        ctx.h2d(self.src8, np.concatenate([_flat(PIXEL8), np.zeros(16, np.uint8)]))
        ctx.h2d(self.src16, np.concatenate([_flat(PIXEL16), np.zeros(16, np.uint8)]))

    def crc(self):
        self.ctx.synchronize()
        self.ctx.d2h(self.out, self.dst)
        return zlib.crc32(self.out.tobytes())

    def close(self):
        for p in (self.src8, self.src16, self.dst):
            self.ctx.free(p)


def _set_flags(mi355fx, ctx, v, sets, fv, fg):
    ctx.set_flag(mi355fx.FLAG_LUT_VARIANT, v)
    ctx.set_flag(mi355fx.FLAG_BRICK_SETS, sets)
    ctx.set_flag(mi355fx.FLAG_FUSED_VARIANT, fv)
    ctx.set_flag(mi355fx.FLAG_FORCE_GENERIC, fg)


def run_product(mi355fx, lut):
    """{case name: [kernel name, CRC-32 of the destination buffer]} of every product case of one LUT, on one context."""
    is3d, size, table = lut_table(lut)
    res = {}
    with mi355fx.Context(0) as ctx:
        ctx.colorlut_load(is3d, size, table)
        B = _Buffers(ctx)
        try:
            for name, entry, v, sets, fv, fg, geom in product_cases():
                w, h, n, pad, gap, off = GEOMS[geom]
                bpp = 4 if entry in ("RGBA", "fused") else 8
                stride = w * bpp + pad
                pitch = stride * (h + gap)
                src = (B.src8 if bpp == 4 else B.src16) + off
                assert off + (n - 1) * pitch + stride * h <= BUF_BYTES
                _set_flags(mi355fx, ctx, v, sets, fv, fg)
                ctx.h2d(B.dst, B.fill)
                if entry == "fused":
                    ctx.hsv_colorlut_frames_device(src, pitch, stride, B.dst, pitch, stride, n, w, h, HSV)
                else:
                    ctx.colorlut_frames_device(src, pitch, stride, B.dst, pitch, stride, n, w, h, entry)
                crc = B.crc()
                res[lut + "/" + name] = [ctx.colorlut_kernel_name(), crc]
        finally:
            B.close()
    return res


AUTO_W, AUTO_H, AUTO_H_BELOW = 256, 256, 252   # 256 x 256 px = 16384 pixel groups = kAutoMinVec exactly; 256 x 252 is below the floor


def run_auto(mi355fx):
    """The measured choice between the arithmetic and the table kernels, from a fresh context: launches of exactly kAutoMinVec pixel
    groups, synchronised one by one (every measurement has arrived when the next launch asks), then one launch below the floor. The
    fused entry and hsvfilter first make the calls their settings need to count as settled. {name: [kernel name or table-in-use, CRC]}."""
    res = {}
    nbytes = AUTO_W * AUTO_H * 4
    src = np.frombuffer(PIXEL8 * (nbytes // 4), np.uint8).copy()
    fill = ((np.arange(nbytes, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)
    out = np.empty(nbytes, np.uint8)

    def sequence(ctx, tag, warm, launch, what):
        d_src, d_dst = ctx.alloc(nbytes), ctx.alloc(nbytes)
        try:
            ctx.h2d(d_src, src)
            steps = [("warm%d" % (i + 1), AUTO_H) for i in range(warm)] + [("auto%d" % (i + 1), AUTO_H) for i in range(4)] + [("below", AUTO_H_BELOW)]
            for step, h in steps:
                ctx.h2d(d_dst, fill)
                launch(ctx, d_src, d_dst, h)
                ctx.synchronize()
                ctx.d2h(out, d_dst)
                res["auto/%s/%s" % (tag, step)] = [what(ctx), zlib.crc32(out.tobytes())]
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)

    def plain(ctx, s, d, h):
        ctx.colorlut_frames_device(s, AUTO_W * h * 4, AUTO_W * 4, d, AUTO_W * h * 4, AUTO_W * 4, 1, AUTO_W, h, "RGBA")

    def fused(ctx, s, d, h):
        ctx.hsv_colorlut_frames_device(s, AUTO_W * h * 4, AUTO_W * 4, d, AUTO_W * h * 4, AUTO_W * 4, 1, AUTO_W, h, HSV)

    def hsv(ctx, s, d, h):   # in place on the destination, which holds the source again before every launch
        ctx.h2d(d, src)
        ctx.hsvfilter_frames_device(d, 1, AUTO_W * h * 4, AUTO_W, h, AUTO_W * 4, "RGBA", HSV)

    for lut in ("3d33", "1d16"):
        for tag, warm, launch in (("plain", 0, plain), ("fused", KSTABLE, fused)):
            with mi355fx.Context(0) as ctx:
                ctx.colorlut_load(*lut_table(lut))
                sequence(ctx, "%s/%s" % (lut, tag), warm, launch, lambda c: c.colorlut_kernel_name())
    for mode in (1, 2):
        with mi355fx.Context(0) as ctx:
            ctx.set_flag(mi355fx.FLAG_HSV_TABLE, mode)
            sequence(ctx, "hsvfilter/mode%d" % mode, KSTABLE, hsv, lambda c: "table" if c.colorlut_kernel_choice(fused=2)[0] else "arithmetic")
    return res


def run_group(mi355fx):
    """One name the single-buffer entry points never set: the multi-frame table kernel of the video group, which
    launch_colorlut_multi (colorlut_kernels.hip) names. Two streams with one LUT, one 128 x 8 frame each, hsvfilter then colorlut."""
    res = {}
    w, h = 128, 8
    fill = prefill()
    out = np.empty(BUF_BYTES, np.uint8)
    ctxs = [mi355fx.Context(0) for _ in range(2)]
    g = mi355fx.Group(0, 8)
    try:
        ptrs = []
        for c in ctxs:
            c.colorlut_load(*lut_table("3d33"))
            s, d = c.alloc(BUF_BYTES), c.alloc(BUF_BYTES)
            c.h2d(s, _flat(PIXEL8))
            c.h2d(d, fill)
            ptrs.append((s, d))
        for t in [g.submit_chain(c, s, d, w, h, w * 4, "RGBA", HSV) for c, (s, d) in zip(ctxs, ptrs)]:
            g.wait(t)
        for i, (c, (s, d)) in enumerate(zip(ctxs, ptrs)):
            c.synchronize()
            c.d2h(out, d)
            res["group/chain/stream%d" % i] = [c.colorlut_kernel_name(), zlib.crc32(out.tobytes())]
            c.free(s)
            c.free(d)
    finally:
        g.close()
        for c in ctxs:
            c.close()
    return res


# Launches whose kernel NAME is a measured choice even with every launch synchronised, so that no recording can pin it: on a 1D LUT
# the fused entry's arithmetic path is hsvfilter + launch_colorlut, and that inner colorlut makes a measured choice of its own. Its
# first four launches of the sequence are compute, compute, table, table; from the fifth on it runs whichever kind measured faster -
# either is right - until the fused entry's own choice turns to its composed table (auto3). The bytes are the same either way:
# the CRC of these launches is compared, the name is not. (Seen as colorlut1d_lds_kernel in the two recordings the golden was made
# from and as colorlut_table_tiled_kernel in a later run of the same host code.)
MEASURED_NAME = "(measured choice)"
MEASURED_CASES = ["auto/1d16/fused/" + s for s in ("warm5", "warm6", "warm7", "warm8", "auto1", "auto2")]


def normalise(results):
    """The form in which recordings and replays are compared: the name of a MEASURED_CASES launch does not count."""
    return {n: [MEASURED_NAME if n in MEASURED_CASES else v[0], v[1]] for n, v in results.items()}


def run_all(mi355fx):
    res = {}
    for lut in LUTS:
        res.update(run_product(mi355fx, lut))
    res.update(run_auto(mi355fx))
    res.update(run_group(mi355fx))
    return normalise(res)


def pack(results):
    """{name: [kernel, crc]} -> the compact form the golden file holds: name tables and one list of index pairs per LUT / sequence."""
    kernels = sorted({v[0] for v in results.values()})
    crcs = sorted({v[1] for v in results.values()})
    ki, ci = {k: i for i, k in enumerate(kernels)}, {c: i for i, c in enumerate(crcs)}
    enc = lambda name: [ki[results[name][0]], ci[results[name][1]]] if name in results else [-1, -1]   # (-1: a dropped case)
    product = {lut: sum((enc(lut + "/" + c[0]) for c in product_cases()), []) for lut in LUTS}   # in product_cases() order, flat
    other = {name: enc(name) for name in results if name.split("/", 1)[0] not in LUTS}
    return {"kernels": kernels, "crcs": crcs, "product": product, "other": other}


def unpack(doc):
    dec = lambda k, c: [doc["kernels"][k], doc["crcs"][c]]
    res = {name: dec(*kc) for name, kc in doc["other"].items()}
    for lut, flat in doc["product"].items():
        names = [lut + "/" + c[0] for c in product_cases()]
        assert len(flat) == 2 * len(names), "the golden was recorded for another case list"
        res.update({n: dec(flat[2 * i], flat[2 * i + 1]) for i, n in enumerate(names) if flat[2 * i] >= 0})
    return res
