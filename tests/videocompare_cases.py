"""The case table of videocompare's five hash kernels (csrc/videocompare_kernels.hip) and a model of their routing: every case names
the branch it is there for, at the smallest frame that reaches it, as data that tests/test_videocompare_cases_cpu.py proves without a
GPU and tests/test_gpu_videocompare_routes.py / test_gpu_group_compare.py replay on one. Plain Python and numpy.

The model restates, from the source:
  route()              the predicate of launch_blockhash / blockhash_enqueue: which sum kernel serves a launch
  splits()             blockhash_rgba_kernel's `split` per lane: how many of a lane's 4 pixels belong to its first block column
  live_lanes()         the lanes of a 1024-pixel segment that hold pixels
  wg_crosses_frames()  the contiguous item range of a workgroup: does one workgroup flush and zero its LDS counters in mid-loop?
  blockhash_bits()     the bit rule of blockhash_finish_kernel, with np.sort: a second opinion beside the C oracle's quick-select
  any_size_bits()      the floating-point path (blockhash_slow_kernel + its host finish) in numpy

Every buffer a case hands to the device is poisoned: row padding, the gap between frames and the bytes before an offset base pointer
hold 0x00 where an alpha byte would sit and 0xEE elsewhere, so a kernel that reads a stray RGBA pixel counts 765 for it (alpha 0 is
white) and one that reads a stray RGB pixel counts 714."""
import zlib

import numpy as np

K_ROW_GROUP = 32          # kRowGroup of blockhash_rgba_kernel
VEC_SEG, BYTES_SEG = 1024, 256
ALL_ONES = 0xFFFFFFFFFFFFFFFF
ALGOS = [("mean", 64), ("gradient", 64), ("vertgradient", 64), ("doublegradient", 40)]


# ------------------------------------------------------------------------------------------------ the model
def route(width, height, channels, stride, frame_pitch, ptr_mod16, n_frames, any_size):
    """Which kernel sums the blocks: "vec" (blockhash_rgba_kernel), "bytes" (blockhash_bytes_kernel), "slow" (blockhash_slow_kernel)
    or "refused". frame_pitch None is the group path (blockhash_enqueue): one launch per frame, no pitch term, no any-size path.
    n_frames is part of the launch, not of the predicate: a single frame with an odd pitch still takes "bytes"."""
    group = frame_pitch is None
    if width <= 0 or height <= 0 or n_frames < 1 or channels not in (3, 4) or stride < width * channels:
        return "refused"
    if width % 8 or height % 8:
        return "slow" if (any_size and not group and width >= 8 and height >= 8) else "refused"
    vec = channels == 4 and stride % 16 == 0 and (group or frame_pitch % 16 == 0) and ptr_mod16 == 0 and width >= 32
    return "vec" if vec else "bytes"


def splits(width):
    """The `split` values below 4 that some lane of the vector kernel sees at this width: the lane's 4 pixels straddle two block
    columns, the first `split` of them go to the left one (acca), the rest to the right one (accb, bin_add_lane)."""
    bw = width // 8
    out = set()
    for x0 in range(0, width, 4):
        split = (x0 // bw + 1) * bw - x0
        if split < 4:
            assert (x0 + 3) // bw == x0 // bw + 1
            out.add(split)
    return out


def live_lanes(width, seg):
    """How many of the 256 lanes of 1024-pixel segment `seg` hold pixels (x0 = seg * 1024 + 4 * lane < width)."""
    return max(0, min(256, (width - seg * VEC_SEG + 3) // 4))


def items_per_frame(kernel, width, height):
    if kernel == "vec":
        return ((height + K_ROW_GROUP - 1) // K_ROW_GROUP) * ((width + VEC_SEG - 1) // VEC_SEG)
    return height * ((width + BYTES_SEG - 1) // BYTES_SEG)


def wg_crosses_frames(n_frames, items_per_frame, n_cu):
    """grid = min(8 * n_cu, total), per_wg = ceil(total / grid), workgroup k owns items [k * per_wg, (k + 1) * per_wg): True when
    some workgroup's range holds items of more than one frame, which is when its loop meets `f != cur_frame` with cur_frame >= 0,
    flushes its 64 LDS counters to the frame it leaves and zeroes them for the one it enters."""
    total = n_frames * items_per_frame
    grid = max(1, min(8 * n_cu, total))
    per_wg = (total + grid - 1) // grid
    for k in range(grid):
        a, b = k * per_wg, min((k + 1) * per_wg, total)
        if a < b and a // items_per_frame != (b - 1) // items_per_frame:
            return True
    return False


def pixel_sums(frame, width, height, channels):
    """sum_px of every pixel: r + g + b, 765 for an RGBA pixel of alpha 0."""
    f = np.asarray(frame, np.uint8).reshape(height, width, channels)
    s = f[..., :3].astype(np.int64).sum(axis=2)
    if channels == 4:
        s[f[..., 3] == 0] = 765
    return s


def block_sums(frame, width, height, channels):
    """The 64 integer block sums of a frame of 8 x 8 whole blocks, block = row * 8 + column."""
    bw, bh = width // 8, height // 8
    return pixel_sums(frame, width, height, channels).reshape(8, bh, 8, bw).sum(axis=(1, 3)).reshape(64)


def blockhash_bits(block_sums, area):
    """The finish rule: two bands of 32, upper median = sorted[16], bit = v > median or (v == median and median > 765 * area // 2)."""
    v = np.asarray(block_sums, np.int64).reshape(64)
    cmp_factor = 765 * area // 2
    bits = 0
    for g in range(2):
        band = v[32 * g: 32 * g + 32]
        median = int(np.sort(band)[16])
        for i in range(32):
            if band[i] > median or (band[i] == median and median > cmp_factor):
                bits |= 1 << (32 * g + i)
    return bits


def any_size_bits(frame, width, height, channels):
    """The floating-point path (sizes not divisible by 8) restated in numpy: every pixel whole to block (floor(x / (w/8)),
    floor(y / (h/8))) with f32 quotients, each block's f32 sum accumulated in row-major pixel order (np.add.accumulate in float32 is
    sequential), upper median of each band of 32, the crate's float comparison."""
    s = pixel_sums(frame, width, height, channels)
    bw, bh = np.float32(width) / np.float32(8), np.float32(height) / np.float32(8)
    bx = np.floor(np.arange(width, dtype=np.float32) / bw).astype(np.int64)
    by = np.floor(np.arange(height, dtype=np.float32) / bh).astype(np.int64)
    blocks = np.zeros(64, np.float32)
    for j in range(8):
        rows = s[by == j]
        for i in range(8):
            vals = rows[:, bx == i].reshape(-1).astype(np.float32)     # row-major within the block = pixel order
            blocks[j * 8 + i] = np.add.accumulate(vals, dtype=np.float32)[-1]
    half = np.float32(765.0) * bw * bh / np.float32(2.0)
    bits = 0
    for g in range(2):
        band = blocks[32 * g: 32 * g + 32]
        median = np.sort(band)[16]
        for i, v in enumerate(band):
            if v > median or (abs(v - median) < 1.0 and median > half):
                bits |= 1 << (32 * g + i)
    return bits


# ------------------------------------------------------------------------------------------------ frames and buffers
def frame_from_levels(levels64, width, height, channels, greedy=False, alpha0_rng=None):
    """A frame of 8 x 8 whole blocks whose block sums are levels64. A block is solid up to one unit: its pixels get sum // area, the
    first sum % area of them one more (greedy: as many pixels of 765 as fit, one pixel with the rest, the others 0). A pixel's
    sum goes to r, then g, then b; alpha is 255. With alpha0_rng (RGBA), every pixel of level 765 is written as alpha 0 over
    random RGB instead: sum_px must still count 765."""
    bw, bh = width // 8, height // 8
    area = bw * bh
    px = np.zeros((64, area), np.int64)
    for b, s in enumerate(np.asarray(levels64).reshape(64)):
        s = int(s)
        assert 0 <= s <= 765 * area
        if greedy:
            q, r = divmod(s, 765)
            px[b, :q] = 765
            if r:
                px[b, q] = r
        else:
            q, r = divmod(s, area)
            px[b] = q
            px[b, :r] += 1
    img = px.reshape(8, 8, bh, bw).transpose(0, 2, 1, 3).reshape(height, width)
    f = np.zeros((height, width, channels), np.uint8)
    f[..., 0] = np.minimum(img, 255)
    f[..., 1] = np.minimum(img - f[..., 0], 255)
    f[..., 2] = img - f[..., 0].astype(np.int64) - f[..., 1]
    if channels == 4:
        f[..., 3] = 255
        if alpha0_rng is not None:
            white = img == 765
            f[white] = alpha0_rng.integers(0, 256, (int(white.sum()), 4), dtype=np.uint8)
            f[white, 3] = 0
    return f.reshape(height, width * channels)


def pack(frames, width, height, channels, stride, pitch, lead=0):
    """The poisoned device buffer of frames (n, height, width * channels): `lead` bytes, then frame k's row y at
    lead + k * pitch + y * stride. Everything that is no pixel holds 0x00 where an alpha byte would sit, 0xEE elsewhere."""
    n = len(frames)
    assert stride >= width * channels and pitch >= stride * height
    idx = np.arange(lead + pitch * n, dtype=np.int64) - lead
    buf = np.full(idx.size, 0xEE, np.uint8)
    if channels == 4:
        buf[((idx % pitch) % stride) % 4 == 3] = 0x00
    body = buf[lead:].reshape(n, pitch)[:, : stride * height].reshape(n, height, stride)
    body[:, :, : width * channels] = np.asarray(frames, np.uint8).reshape(n, height, width * channels)
    return buf


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def random_frames(key, n, width, height, channels):
    """n distinct frames as the suite's random frames are: uniform bytes, the top half darkened so that the two bands' medians
    separate, 10 % of an RGBA frame's pixels fully transparent."""
    rng = _rng(key)
    f = rng.integers(0, 256, (n, height, width, channels), dtype=np.uint8)
    f[:, : height // 2] //= 3
    if channels == 4:
        f[..., 3] = np.where(rng.random((n, height, width)) < 0.1, 0, 255)
    return f.reshape(n, height, width * channels)


def column_frame(width, height, channels):
    """Pixel columns alternate 0 and 255: a pixel booked to the wrong side of a block edge changes two block sums by 765."""
    f = np.zeros((height, width, channels), np.uint8)
    f[:, 1::2, :3] = 255
    if channels == 4:
        f[..., 3] = 255
    return f.reshape(1, height, width * channels)


def rotated_frames(key, n, width, height, channels):
    """Frame k has the 64 block levels (a fixed permutation of the greys 0, 4, .. 252) rotated by k, with 2 random low bits per
    byte: neighbours differ in every block, so counters that leak from one frame into the next change its sums."""
    rng = _rng(key)
    bw, bh = width // 8, height // 8
    levels = ((np.arange(64)[None, :] + np.arange(n)[:, None]) % 64) * 37 % 64
    grey = (levels * 4).astype(np.uint8).reshape(n, 8, 1, 8, 1)
    img = np.broadcast_to(grey, (n, 8, bh, 8, bw)).reshape(n, height, width, 1)
    f = np.broadcast_to(img, (n, height, width, channels)) | rng.integers(0, 4, (n, height, width, channels), dtype=np.uint8)
    f = np.ascontiguousarray(f)
    if channels == 4:
        f[..., 3] = 255
    return f.reshape(n, height, width * channels)


def ramp_frame(rng, width, height, channels):
    """The ramp-xor-noise frame of test_resize_based_hashes_match_oracle; an RGBA frame carries random alpha (luma ignores it)."""
    yy, xx = np.mgrid[0:height, 0:width]
    f = np.zeros((height, width, channels), np.uint8)
    f[..., 0] = (xx * 255 // max(width - 1, 1)) ^ rng.integers(0, 32, (height, width))
    f[..., 1] = yy * 255 // max(height - 1, 1)
    f[..., 2] = rng.integers(0, 256, (height, width))
    return f


def _grey(img, channels, rng):
    f = np.repeat(np.asarray(img, np.uint8)[..., None], channels, axis=2)
    if channels == 4:
        f[..., 3] = rng.integers(0, 256, img.shape)
    return f


class Case:
    """One launch: n_frames frames of one geometry at base pointer `lead` bytes past a 16-byte boundary. `kernel` is the claimed
    route; `pixels` keys the pixel content, so cases that share it hash the same frames through different routes."""

    def __init__(self, id, width, height, channels, stride=None, pitch=None, lead=0, n_frames=3, content="random", kernel=None, pixels=None,
                 any_size=False, **claims):
        self.id, self.width, self.height, self.channels = id, width, height, channels
        self.stride = width * channels if stride is None else stride
        self.pitch = self.stride * height if pitch is None else pitch
        self.lead, self.n_frames, self.content, self.kernel, self.any_size = lead, n_frames, content, kernel, any_size
        self.pixels = pixels or id
        self.claims = claims

    fmt = property(lambda self: "RGBA" if self.channels == 4 else "RGB")
    area = property(lambda self: (self.width // 8) * (self.height // 8))
    padded = property(lambda self: self.stride > self.width * self.channels or self.pitch > self.stride * self.height or self.lead > 0)

    def route(self):
        return route(self.width, self.height, self.channels, self.stride, self.pitch, self.lead % 16, self.n_frames, self.any_size)

    def frames(self):
        w, h, c, n = self.width, self.height, self.channels, self.n_frames
        kind = self.content
        if kind == "random":
            return random_frames(self.pixels, n, w, h, c)
        if kind == "random+columns":
            return np.concatenate([random_frames(self.pixels, n - 1, w, h, c), column_frame(w, h, c)])
        if kind == "rotated":
            return rotated_frames(self.pixels, n, w, h, c)
        if kind == "solids":
            return np.stack([np.tile(np.array(rgb + (255,), np.uint8)[:c], (h, w)) for rgb in ((255, 255, 255), (128, 128, 127), (10, 10, 10))])
        if kind == "levels":
            rng = _rng(self.pixels)
            return np.stack([frame_from_levels(s, w, h, c, greedy=self.claims.get("greedy", False), alpha0_rng=rng if self.claims.get("alpha0") else None)
                             for s in self.claims["sums"](765 * self.area // 2, self.area)])
        return resize_frames(kind, self.pixels, w, h, c)


def resize_frames(kind, key, w, h, c):
    """The content sets of the resize-based hashes, three distinct frames each; every RGBA frame carries random alpha."""
    rng = _rng(key)
    if kind == "ramps":
        fs = []
        for _ in range(3):
            f = ramp_frame(rng, w, h, c)
            if c == 4:
                f[..., 3] = rng.integers(0, 256, (h, w))
            fs.append(f)
    elif kind == "solid":
        fs = [_grey(np.full((h, w), v), c, rng) for v in (0, 77, 255)]
    elif kind == "halves":
        lr, tb = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        lr[:, w // 2:] = 255
        tb[h // 2:] = 255
        fs = [_grey(lr, c, rng), _grey(tb, c, rng), _grey(255 - lr, c, rng)]
    else:
        assert kind.startswith("checker")
        p = int(kind[7:])
        yy, xx = np.mgrid[0:h, 0:w]
        board = (((yy // p) + (xx // p)) % 2 * 255).astype(np.uint8)
        fs = [_grey(board, c, rng), _grey(255 - board, c, rng), _grey(np.roll(board, p // 2, axis=1), c, rng)]
    return np.stack(fs).reshape(3, h, w * c)


# ------------------------------------------------------------------------------------------------ routes
_R1 = dict(width=40, height=16, channels=4, pixels="R1")
ROUTE_CASES = [
    # R1: the vector kernel with padded rows and a gap between frames; R2..R4 leave it by exactly one term of the predicate
    Case("R1-vec-padded-gap", stride=176, pitch=176 * 16 + 32, kernel="vec", **_R1),
    Case("R2-stride+4", stride=180, pitch=180 * 16 + 32, kernel="bytes", term="stride", **_R1),
    Case("R3-pitch+8", stride=176, pitch=176 * 16 + 40, kernel="bytes", term="pitch", **_R1),
    Case("R4-pointer+4", stride=176, pitch=176 * 16 + 32, lead=4, kernel="bytes", term="pointer", **_R1),
    # R5: narrow frames (block width below 4) take bytes whatever their alignment
    Case("R5-8x8", 8, 8, 4, kernel="bytes", term="width"),
    Case("R5-16x8", 16, 8, 4, kernel="bytes", term="width"),
    Case("R5-24x8", 24, 8, 4, kernel="bytes", term="width"),
    Case("R5-24x16-rgb", 24, 16, 3, stride=24 * 3 + 5, pitch=(24 * 3 + 5) * 16 + 7, kernel="bytes", term="channels"),
    # R6: RGB never takes vec, packed (stride 120, not a multiple of 16) or padded to one (128)
    Case("R6-rgb-packed", 40, 48, 3, kernel="bytes", term="channels", pixels="R6"),
    Case("R6-rgb-padded", 40, 48, 3, stride=128, pitch=128 * 48 + 16, kernel="bytes", term="channels", pixels="R6"),
]

# ------------------------------------------------------------------------------------------------ lane split
SPLIT_WIDTHS = [40, 48, 56, 200]        # block widths 5, 6, 7, 25
SPLIT_HEIGHTS = [8, 40, 264]            # 8: block height 1, a flush every row; 40: two row groups, the second 8 rows; 264: block height 33
SPLIT_CASES = [Case("split-%dx%d" % (w, h), w, h, 4, content="random+columns", kernel="vec", pixels="split-%d-%d" % (w, h))
               for w in SPLIT_WIDTHS for h in SPLIT_HEIGHTS]
# the second / third 1024-pixel segment has 2 live lanes: its first wave holds live and dead lanes (bin >= 0 and -1 in one bin_add)
SPLIT_CASES += [Case("split-1032x8", 1032, 8, 4, content="random+columns", kernel="vec", segments=2, last_live=2),
                Case("split-2056x16", 2056, 16, 4, content="random+columns", kernel="vec", segments=3, last_live=2)]

# ------------------------------------------------------------------------------------------------ several frames per workgroup
# (case, ladder of frame counts): at every CU count from 1 to 512 some rung has wg_crosses_frames() true
LADDERS = [
    ("wg-vec-32x72", dict(width=32, height=72, channels=4, kernel="vec"), [300, 900, 1400]),      # 3 items per frame, block height 9
    # 8 items per frame. 100 and 600 alone leave 274 CU counts (75 up) at which per_wg divides 8 and every workgroup stays inside one
    # frame; 700 and 1050 close them
    ("wg-bytes-16x8-rgb", dict(width=16, height=8, channels=3, kernel="bytes"), [100, 600, 700, 1050]),
]
LADDER_CASES = [Case("%s-x%d" % (name, n), n_frames=n, content="rotated", pixels=name, **geom) for name, geom, rungs in LADDERS for n in rungs]


# ------------------------------------------------------------------------------------------------ finish rule
PERM = [(13 * i + 5) % 32 for i in range(32)]      # a fixed permutation of the 32 lanes of a band (13 is odd: a bijection)
ORDERS = {"ascending": list(range(32)), "descending": list(range(31, -1, -1)), "permuted": PERM}


def band_f2(low, high):
    """16 low, 16 high: columns 0..3 of every block row high. The upper median is the high value."""
    return [high if i % 8 < 4 else low for i in range(32)]


def band_f3(k, tied):
    """Ascending: 15 below, k at the median, 17 - k above."""
    return [tied - 1 - 3 * j for j in range(14, -1, -1)] + [tied] * k + [tied + 1 + 5 * j for j in range(17 - k)]


def band_f4(low):
    """Ascending: 17 equal low, 15 high. The median is the low value."""
    return [low] * 17 + [low + 1 + 5 * j for j in range(15)]


def _ordered(band, order):
    return [band[i] for i in ORDERS[order]]


def _both(band0, band1=None):
    return np.array(list(band0) + list(band0[::-1] if band1 is None else band1), np.int64)


def _f1(c, a):
    return [np.full(64, c - 1), np.full(64, c), np.full(64, c + 1)]


def _f2(c, a):
    return [_both(band_f2(30 * a, 600 * a), band_f2(30 * a, 600 * a)), _both(band_f2(30 * a, 300 * a), band_f2(30 * a, 300 * a))]


def _f3(k):
    return lambda c, a: [_both(band_f3(k, t)) for t in (c + 1, c, c - 1)]


def _f4(c, a):
    return [_both(band_f4(c + 1)), _both(band_f4(c))]


def _f5(c, a):
    return [_both(band_f3(3, c + 40), _ordered(band_f3(3, c - 40), "descending")), _both(band_f3(4, c - 40), _ordered(band_f3(2, c + 40), "permuted"))]


def _f6(bands):
    return lambda c, a: [_both(_ordered(b, o), _ordered(b, o)) for b in bands(c, a) for o in ORDERS]


def _f7(c, a):
    return _f1(c, a) + [np.full(64, 765 * a)]


FINISH_SIZES = [(8, 8, "bytes"), (24, 8, "bytes"), (64, 8, "vec")]     # areas 1, 3 (765 * 3 / 2 = 1147.5 -> 1147), 8
# name: (block sums of each frame as a function of (cmp_factor, area), literal hashes or None, greedy / alpha-0 writing)
FINISH_FRAMES = {
    "F1-all-equal-around-half": (_f1, [0, 0, ALL_ONES], {}),
    "F2-16-low-16-high": (_f2, [0x0F0F0F0F0F0F0F0F, 0], {}),
    "F3-tied-median-k2": (_f3(2), None, {}), "F3-tied-median-k3": (_f3(3), None, {}),
    "F3-tied-median-k4": (_f3(4), None, {}), "F3-tied-median-k5": (_f3(5), None, {}),
    "F4-17-low-15-high": (_f4, None, {}),
    "F5-bright-band-dark-band": (_f5, None, {}),
    "F6-F2-orders": (_f6(lambda c, a: [sorted(band_f2(30 * a, 600 * a)), sorted(band_f2(30 * a, 300 * a))]), None, {}),
    "F6-F3-orders": (_f6(lambda c, a: [band_f3(k, t) for k in (2, 3, 4, 5) for t in (c + 1, c)]), None, {}),
    "F6-F4-orders": (_f6(lambda c, a: [band_f4(c + 1), band_f4(c)]), None, {}),
    # F1's three sums and full white, reached with as many pixels of level 765 as fit, each written as alpha 0 over random RGB (at
    # area 1 only the white frame has such a pixel)
    "F7-alpha0-is-white": (_f7, [0, 0, ALL_ONES, ALL_ONES], {"greedy": True, "alpha0": True}),
}
FINISH_CASES = []
for _name, (_sums, _lit, _kw) in FINISH_FRAMES.items():
    for _w, _h, _k in FINISH_SIZES:
        _n = len(_sums(765 * (_w // 8) * (_h // 8) // 2, (_w // 8) * (_h // 8)))
        FINISH_CASES.append(Case("%s-%dx%d" % (_name, _w, _h), _w, _h, 4, n_frames=_n, content="levels", kernel=_k, sums=_sums, literals=_lit, **_kw))

# ------------------------------------------------------------------------------------------------ any-size path
ANY_SIZE_CASES = [
    Case("any-9x8", 9, 8, 4, stride=9 * 4 + 12, pitch=(9 * 4 + 12) * 8 + 9, kernel="slow", any_size=True),
    Case("any-12x12", 12, 12, 4, stride=12 * 4 + 12, pitch=(12 * 4 + 12) * 12 + 9, kernel="slow", any_size=True),
    Case("any-17x23-rgb", 17, 23, 3, stride=17 * 3 + 5, pitch=(17 * 3 + 5) * 23 + 9, kernel="slow", any_size=True),
    Case("any-20x12", 20, 12, 4, stride=20 * 4 + 12, pitch=(20 * 4 + 12) * 12 + 9, kernel="slow", any_size=True),
    # solid white, (128, 128, 127) and (10, 10, 10): blocks of equal pixel count tie, |v - median| < 1 && median > half decides
    Case("any-12x12-solids", 12, 12, 4, stride=12 * 4 + 12, pitch=(12 * 4 + 12) * 12 + 9, content="solids", kernel="slow", any_size=True),
    Case("any-20x12-solids", 20, 12, 4, stride=20 * 4 + 12, pitch=(20 * 4 + 12) * 12 + 9, content="solids", kernel="slow", any_size=True),
]

# ------------------------------------------------------------------------------------------------ resize-based hashes
RESIZE_SIZES = [(257, 9), (9, 257), (3, 2), (1, 1), (40, 24)]      # 257 x 9: the vertical kernel's second 256-wide block has one live lane
CHECKER = "checker8"                                                # the board pitch whose resized image saturates at both ends (CPU test)
RESIZE_CASES = []
for _w, _h in RESIZE_SIZES:
    for _c, _pad in ((4, 16), (3, 5)):
        for _content in ["ramps", "solid", "halves"] + ([CHECKER] if (_w, _h) == (40, 24) else []):
            _s = _w * _c + _pad
            RESIZE_CASES.append(Case("resize-%dx%d-%s-%s" % (_w, _h, "rgba" if _c == 4 else "rgb", _content), _w, _h, _c, stride=_s,
                                     pitch=_s * _h + 24, content=_content, kernel="imghash"))

# ------------------------------------------------------------------------------------------------ distance
DISTANCE_CASES = [("blockhash", 0, ALL_ONES, 64.0), ("blockhash", 1 << 63, 0, 1.0), ("doublegradient", 0xA5A5A5A5A5, 0x5A5AA5A5A4, None)]

# ------------------------------------------------------------------------------------------------ the group path (blockhash_enqueue)
# (id, width, height, stride, bytes the second frame's pointer is past a 16-byte boundary, kernel of the reference, kernel of the frame)
GROUP_CASES = [
    ("padded-stride", 40, 16, 176, 0, "vec", "vec"),
    ("second-frame-pointer+4", 40, 16, 160, 4, "vec", "bytes"),     # one pair mixes the two kernels
    ("narrow", 24, 16, 96, 0, "bytes", "bytes"),
]
