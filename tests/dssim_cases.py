"""The case table of the exact Dssim engine (csrc/dssim_kernels.hip) and a model of its routing: every geometry names the branch it
is there for, at the smallest frame that reaches it, as data that tests/test_dssim_cases_cpu.py proves without a GPU and
tests/test_gpu_dssim_routes.py / test_gpu_group_compare.py replay on one. Plain Python and numpy.

The model restates, from the source:
  scale_chain()        dssim_create_image's geometry loop: halve while w >= 8 and h >= 8, at most five scales
  tiles()              blocks of a tile kernel over one scale
  interior_tiles()     the block-uniform INTERIOR test of the three tile kernels: the tile plus its halo lies inside the scale. The scale
                       and hash-compare kernels have halo 4 (tx, ty >= 1, 32 tx + 36 <= w, 16 ty + 20 <= h), the compare kernel halo 2
  launches()           scales 0 and 1 get a launch each, scales 2.. share one of up to three jobs with first[]
  u8_form()            the byte-load form of dssim_downsample_u8_kernel: "wide" (RGBA, pointer % 8 == 0, stride % 8 == 0), "bytes", "rgb"
  grid_blocks()        the grid of the 256-lane grid-stride kernels (box chain, absolute deviations): one block per 256, at most 8 n_cu
  avg_eight_load_lanes() / absdev_trips()   which lanes of dssim_avg_kernel enter its eight-load loop; trips of the absdev loop
  plan()               all of it for one frame size, in the shape of mi355fx.selftest_dssim_plan
The tile constants come from the library (mi355_selftest_dssim_plan), never from literals here.

Every buffer a case hands to the device is poisoned as tests/dssim_f64.make_case does: row padding and the bytes before an offset
base pointer hold 0xA5."""
import os
import subprocess
import zlib

import numpy as np

MAX_SCALES = 5
POISON = 0xA5
_consts = None


def constants():
    """(tile_w, tile_h, tile_lanes, scale_halo, compare_halo) as the library was built."""
    global _consts
    if _consts is None:
        import mi355fx
        if not os.path.exists(mi355fx.LIB_PATH):
            subprocess.check_call(["make", "-s", "-C", mi355fx.PKG_ROOT])
        rc, p = mi355fx.selftest_dssim_plan(8, 8, 1)
        assert rc == 0
        _consts = p["tile"]
    return _consts


TW, TH, NT, HALO, CHALO = constants()


# ------------------------------------------------------------------------------------------------ the model
def scale_chain(w, h):
    out = [(w, h)]
    while len(out) < MAX_SCALES and w >= 8 and h >= 8:
        w, h = w // 2, h // 2
        out.append((w, h))
    return out


def tiles(w, h):
    return ((w + TW - 1) // TW) * ((h + TH - 1) // TH)


def interior_tiles(w, h, halo):
    """[(tx, ty, touches_right, touches_bottom)] of the tiles whose region (tile + halo) lies inside a w x h scale; `touches`: the
    region ends exactly on the last column / row (the kernels' <= is an equality)."""
    out = []
    for ty in range((h + TH - 1) // TH):
        for tx in range((w + TW - 1) // TW):
            x0, y0 = tx * TW - halo, ty * TH - halo
            x1, y1 = x0 + TW + 2 * halo, y0 + TH + 2 * halo
            if x0 >= 0 and y0 >= 0 and x1 <= w and y1 <= h:
                out.append((tx, ty, x1 == w, y1 == h))
    return out


def launches(chain):
    """[(first scale, jobs, first[0..3])]: blocks [first[j], first[j + 1]) of the launch belong to scale first_scale + j."""
    out, k, ns = [], 0, len(chain)
    while k < ns:
        count = 1 if k < 2 else min(3, ns - k)
        first, total = [], 0
        for j in range(3):
            first.append(total)
            if j < count:
                total += tiles(*chain[k + j])
        out.append((k, count, tuple(first + [total])))
        k += count
    return out


def u8_form(channels, pointer, stride):
    if channels == 3:
        return "rgb"
    return "wide" if pointer % 8 == 0 and stride % 8 == 0 else "bytes"


def grid_blocks(n_cu, n):
    return max(1, min((n + 255) // 256, 8 * n_cu))


def avg_eight_load_lanes(n_partials):
    """Lanes of dssim_avg_kernel's one block that enter `for (; i + 7 * 256 < n_a; ...)` at i = lane."""
    return max(0, min(256, n_partials - 7 * 256))


def absdev_trips(n, blocks):
    """Trips of lane 0 of block 0 through dssim_absdev2_kernel's grid-stride loop."""
    return (n + blocks * 256 - 1) // (blocks * 256)


def plan(w, h, n_cu=256):
    chain = scale_chain(w, h)
    return dict(tile=(TW, TH, NT, HALO, CHALO), scales=chain, tiles=[tiles(*s) for s in chain],
                interior_scale=[len(interior_tiles(sw, sh, HALO)) for sw, sh in chain],
                interior_compare=[len(interior_tiles(sw, sh, CHALO)) for sw, sh in chain],
                downsample_blocks=[grid_blocks(n_cu, sw * sh) if k else 0 for k, (sw, sh) in enumerate(chain)],
                absdev_blocks=[grid_blocks(n_cu, sw * sh) for sw, sh in chain], launches=launches(chain),
                avg_blocks=len(chain), sum_blocks=len(chain))


# ------------------------------------------------------------------------------------------------ contents
def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def _opaque(rgb):
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, rgb.dtype)], -1)


def _noise(key, w, h, amp):
    rng = _rng("noise-%s" % key)                      # the reference frame depends on the geometry alone: amplitudes share it
    ref = rng.integers(0, 256, (h, w, 3))
    mod = np.clip(ref + _rng("noise-%s-%d" % (key, amp)).integers(-amp, amp + 1, (h, w, 3)), 0, 255)
    return ref, mod


def _translucent_alpha(rng, w, h):
    return rng.choice(np.array([0, 1, 254, 255]), (h, w), p=[0.1, 0.1, 0.1, 0.7])


def content_pixels(content, w, h, channels):
    """-> (ref, mod) as (h, w, channels) uint8 arrays."""
    key = "%dx%d" % (w, h)
    if content in ("noise3", "noise40", "identical"):
        ref, mod = _noise(key, w, h, {"noise3": 3, "noise40": 40, "identical": 0}[content])
    elif content == "inverted":
        blocks = _rng("inverted-" + key).integers(0, 2, ((h + 15) // 16, (w + 15) // 16))
        ref = np.kron(blocks, np.ones((16, 16), np.int64))[:h, :w, None].repeat(3, axis=2) * 255
        mod = 255 - ref
    elif content == "threshold":
        rng = _rng("threshold-" + key)
        ref, mod = rng.integers(20, 28, (h, w, 3)), rng.integers(20, 28, (h, w, 3))
    elif content in ("translucent", "translucent-black"):
        assert channels == 4
        rng = _rng("translucent-" + key)
        ref, mod = _noise(key, w, h, 40)
        ref = np.concatenate([ref, _translucent_alpha(rng, w, h)[..., None]], -1)
        mod = np.concatenate([mod, _translucent_alpha(rng, w, h)[..., None]], -1)
        return ref.astype(np.uint8), mod.astype(np.uint8)
    else:
        raise ValueError(content)
    ref, mod = ref.astype(np.uint8), mod.astype(np.uint8)
    return (_opaque(ref), _opaque(mod)) if channels == 4 else (ref, mod)


def pack(px, stride, lead):
    """The poisoned buffer of one frame: `lead` bytes, then row y at lead + y * stride; every byte that is no pixel holds 0xA5."""
    h, w, ch = px.shape
    assert stride >= w * ch
    buf = np.full(lead + h * stride, POISON, np.uint8)
    buf[lead:].reshape(h, stride)[:, : w * ch] = px.reshape(h, w * ch)
    return buf


class Case:
    """One (reference, modified) pair of one geometry. `layout` names the byte layout the device entries see: channels, row padding
    and the offset of the base pointer from its allocation. `ref_key`: cases of a geometry with the same key share the reference frame
    and the layout."""
    LAYOUTS = {
        "rgba": (4, 12, 0),          # stride % 8 is 4 for an even width, 0 for an odd one
        "rgb": (3, 5, 0),
        "rgba-wide": (4, 8, 0),      # even widths: pointer % 8 == 0 and stride % 8 == 0
        "rgba-stride4": (4, 4, 0),   # even widths: stride % 8 == 4
        "rgba-base4": (4, 8, 4),     # even widths: stride % 8 == 0, pointer = allocation + 4
    }

    def __init__(self, w, h, content, layout="rgba", pattern=True):
        self.w, self.h, self.content, self.layout, self.pattern = w, h, content, layout, pattern
        self.channels, pad, self.lead = self.LAYOUTS[layout]
        self.stride = w * self.channels + pad
        self.id = "%dx%d-%s-%s" % (w, h, content, layout)
        base = "noise" if content in ("noise3", "noise40", "identical") else content
        self.ref_key = (base, layout, pattern)

    fmt = property(lambda self: "RGBA" if self.channels == 4 else "RGB")

    def pixels(self):
        return content_pixels(self.content, self.w, self.h, self.channels)

    def buffers(self):
        """(ref, mod): flat poisoned uint8 buffers; the frame starts `lead` bytes in."""
        ref, mod = self.pixels()
        return pack(ref, self.stride, self.lead), pack(mod, self.stride, self.lead)

    def device_form(self, allocation=0):
        """The byte-load form dssim_downsample_u8_kernel takes for this case through the device entry points."""
        return u8_form(self.channels, allocation + self.lead, self.stride)

    def host_form(self):
        """... and through the host entry points, which upload the rows packed to an aligned staging buffer."""
        return u8_form(self.channels, 0, self.w * self.channels)


BASIC = [("noise3", "rgba"), ("noise40", "rgba"), ("identical", "rgba"), ("noise40", "rgb")]
FULL = BASIC + [("inverted", "rgba"), ("threshold", "rgba"), ("translucent", "rgba", True), ("translucent-black", "rgba", False),
                ("noise40", "rgba-wide"), ("noise40", "rgba-stride4"), ("noise40", "rgba-base4")]
LONE = [("noise40", "rgba")]


class Geometry:
    """A frame size, the branch it is in the table for, what the model must say about it (`claims`, proved by the CPU test), and the
    contents it is run with."""

    def __init__(self, w, h, branch, contents=BASIC, **claims):
        self.w, self.h, self.branch, self.claims = w, h, branch, claims
        self.id = "%dx%d" % (w, h)
        self.cases = [Case(w, h, *c) for c in contents]

    def groups(self):
        """The cases that one compare_frames / pairs call can take together - one byte layout, one setting of the translucency flag -
        in table order."""
        out = {}
        for c in self.cases:
            out.setdefault((c.layout, c.pattern), []).append(c)
        return list(out.values())


# ------------------------------------------------------------------------------------------------ the table
# claims: scales = number of scales; last = size of the last scale; size1 = size of scale 1; tiles0 = tiles of scale 0;
# interior = {scale: (tiles INTERIOR under the scale / hash-compare kernels' halo, under the compare kernel's)};
# touch_scale / touch_compare = {scale: (tx, ty)}: that tile is interior there and its region ends on the last column AND row;
# spare_scale / spare_compare = {scale: (tx, ty)}: interior with a column and a row to spare;
# grouped = first[] of the launch that serves scales 2..; avg_lanes = lanes of dssim_avg_kernel in its eight-load loop at scale 0;
# absdev = (blocks, trips) of scale 0 at n_cu <= 256
BELOW_HALO = [Geometry(w, h, "below the halo: one scale, every tap clamps", scales=1, tiles0=t, interior={0: (0, 0)}, narrower_than_halo=True)
              for w, h, t in ((1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (3, 40, 3))]
CHAIN_ENDS = [
    Geometry(7, 7, "scale chain: 7 < 8 stops it at once", scales=1),
    Geometry(8, 8, "scale chain: 8 halves once", scales=2, size1=(4, 4), last=(4, 4)),
    Geometry(8, 7, "scale chain: one side below 8 stops it", scales=1),
    Geometry(15, 15, "scale chain: 15 halves once, to 7", scales=2, size1=(7, 7), last=(7, 7)),
    Geometry(16, 16, "scale chain: three scales, the grouped launch has one job", scales=3, last=(4, 4), grouped=(0, 1, 1, 1)),
    Geometry(32, 32, "scale chain: four scales, the grouped launch has two jobs", scales=4, last=(4, 4), grouped=(0, 1, 2, 2)),
    Geometry(64, 64, "scale chain: five scales ending at 4x4, three one-tile jobs in the grouped launch", scales=5, last=(4, 4), grouped=(0, 1, 2, 3)),
    Geometry(128, 128, "scale chain: stopped by the cap of five at 8x8", scales=5, last=(8, 8), grouped=(0, 2, 3, 4)),
    Geometry(37, 19, "scale chain: odd sizes lose a column and a row per halving", scales=3, size1=(18, 9), last=(9, 4)),
    Geometry(17, 9, "scale chain: odd sizes lose a column and a row per halving", scales=2, size1=(8, 4), last=(8, 4)),
]
EDGE_OFFSETS = ((-2, -2), (-1, -1), (1, 1), (2, 2), (-2, 1), (-1, 2), (1, -2), (2, -1))     # those of tests/test_gpu_dssim_fast.py
TILE_EDGES = [Geometry(TW + dx, TH + dy, "tile edge: %+d columns, %+d rows around one tile" % (dx, dy),
                       tiles0=(2 if dx > 0 else 1) * (2 if dy > 0 else 1), interior={0: (0, 0)}) for dx, dy in EDGE_OFFSETS]
_SX, _SY = 2 * TW + HALO, 2 * TH + HALO         # 68 x 36: the smallest scale with a tile INTERIOR under halo 4
_CX, _CY = 2 * TW + CHALO, 2 * TH + CHALO       # 66 x 34: ... under halo 2
THRESHOLDS = [
    Geometry(_SX - 1, _SY, "scale / hash-compare interior: one column short", interior={0: (0, 1)}),
    Geometry(_SX, _SY - 1, "scale / hash-compare interior: one row short", interior={0: (0, 1)}),
    Geometry(_SX, _SY, "scale / hash-compare interior: one tile, ends on the last column and row", FULL, interior={0: (1, 1)},
             touch_scale={0: (1, 1)}, spare_compare={0: (1, 1)}),
    Geometry(_SX + 1, _SY + 1, "scale / hash-compare interior: one tile, a column and a row to spare", interior={0: (1, 1)},
             spare_scale={0: (1, 1)}),
    Geometry(_CX - 1, _CY, "compare interior: one column short", interior={0: (0, 0)}),
    Geometry(_CX, _CY - 1, "compare interior: one row short", interior={0: (0, 0)}),
    Geometry(_CX, _CY, "compare interior: one tile, ends on the last column and row", interior={0: (0, 1)}, touch_compare={0: (1, 1)}),
    Geometry(_CX + 1, _CY + 1, "compare interior: one tile, a column and a row to spare", interior={0: (0, 1)}, spare_compare={0: (1, 1)}),
]
OTHER_SCALES = [
    Geometry(4 * TW + HALO, 4 * TH + HALO, "touching in tile (3, 3) of scale 0; the compare kernel touches at scale 1", FULL,
             touch_scale={0: (3, 3)}, touch_compare={1: (1, 1)}, size1=(_CX, _CY)),
    Geometry(2 * _SX, 2 * _SY, "touching at scale 1: the float4-source interior path", size1=(_SX, _SY), touch_scale={1: (1, 1)}),
    Geometry(4 * _SX, 4 * _SY, "touching at scale 2: an interior tile in job 0 of a grouped launch", FULL, touch_scale={2: (1, 1)},
             grouped=(0, 9, 13, 14)),
]
REDUCTIONS = [
    Geometry(7 * 256 * TW, 1, "dssim_avg_kernel: the last tile count that skips the eight-load loop", LONE, scales=1, tiles0=1792, avg_lanes=0),
    Geometry(7 * 256 * TW + 1, 1, "dssim_avg_kernel: the first tile count that enters the eight-load loop (lane 0 alone)", LONE, scales=1,
             tiles0=1793, avg_lanes=1),
    Geometry(7, 74899, "dssim_absdev2_kernel: the grid at its cap of 8 n_cu blocks, a second trip of the grid-stride loop", LONE, scales=1,
             absdev=(2048, 2)),
]
GEOMETRIES = BELOW_HALO + CHAIN_ENDS + TILE_EDGES + THRESHOLDS + OTHER_SCALES + REDUCTIONS
FULL_GEOMETRIES = [g for g in GEOMETRIES if len(g.cases) == len(FULL)]
GROUP_GEOMETRIES = THRESHOLDS           # test_gpu_group_compare.py: the eight of them in one interval of the compare queue
# scales whose mean SSIM the inverted-blocks content drives below zero (the clamp of dssim_avg_kernel)
NEGATIVE_MEAN = {"68x36": (2, 3), "132x68": (1, 2, 3, 4), "272x144": (1, 2, 3, 4)}


# ------------------------------------------------------------------------------------------------ the restatement of a case
_reference = {}


def reference(case):
    """(value, [SSIM map per scale], image of the reference frame, image of the modified frame) under oracle/dssim_restate.py:
    computed once per case, shared, never changed."""
    if case.id not in _reference:
        from oracle import dssim_restate as D
        ref, mod = case.buffers()
        a = D.DssimImage(ref[case.lead:], case.w, case.h, case.stride, case.channels, case.pattern)
        b = D.DssimImage(mod[case.lead:], case.w, case.h, case.stride, case.channels, case.pattern)
        d, maps = D.compare(a, b, return_maps=True)
        _reference[case.id] = (float(d), maps, a, b)
    return _reference[case.id]


def lab_inputs(px):
    """fx, fy, fz of an opaque frame at scale 0 - what dssim_f / dssim_f_pair select on - in the restatement's arithmetic."""
    from oracle import dssim_restate as D
    F = D.F
    h, w, ch = px.shape
    lin = D.to_linear(px.reshape(-1), w, h, w * ch, ch)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    def mat(rx, gx, bx, d):
        return (r * (F(rx) / d) + g * (F(gx) / d)) + b * (F(bx) / d)
    return mat(0.4124, 0.3576, 0.1805, D.D65[0]), mat(0.2126, 0.7152, 0.0722, D.D65[1]), mat(0.0193, 0.1192, 0.9505, D.D65[2])
