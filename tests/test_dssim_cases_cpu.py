"""The case table of the exact Dssim engine (tests/dssim_cases.py) is proved here, without a GPU: the routing model equals the
library's own plan (mi355_selftest_dssim_plan: the functions and constants the launches use) on every case and on a sweep, the
scale shapes are the restatement's, and every claim a geometry makes - which branch it reaches, and that a neighbouring size does
not - holds. Editing a claim to a neighbouring size fails here: test_gpu_dssim_routes.py then runs what the table says."""
import numpy as np
import pytest

import dssim_cases as T

N_CUS = (1, 8, 256, 304)


def _lib_plan(w, h, n_cu):
    import mi355fx
    rc, p = mi355fx.selftest_dssim_plan(w, h, n_cu)
    assert rc == 0
    return p


@pytest.mark.parametrize("g", T.GEOMETRIES, ids=[g.id for g in T.GEOMETRIES])
def test_the_model_is_the_librarys_plan_on_every_case(g):
    for n_cu in N_CUS:
        assert T.plan(g.w, g.h, n_cu) == _lib_plan(g.w, g.h, n_cu), n_cu


def test_the_model_is_the_librarys_plan_on_a_sweep_and_bad_arguments_are_refused():
    import mi355fx
    for w in range(1, 81):
        for h in range(1, 81):
            assert T.plan(w, h, 8) == _lib_plan(w, h, 8), (w, h)
    for w, h in ((3840, 2160), (1920, 1080), (641, 363)):
        assert T.plan(w, h, 256) == _lib_plan(w, h, 256)
    for args in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)):
        assert mi355fx.selftest_dssim_plan(*args) == (mi355fx.ERR_INVALID_ARG, None)
    assert mi355fx.load_library().mi355_selftest_dssim_plan(8, 8, 8, None) == mi355fx.ERR_INVALID_ARG


def test_the_tile_constants_are_the_ones_the_documents_state():
    """32 x 16 tiles of 256 lanes, halo 4 / 2: what csrc/dssim_kernels.hip's comments and DESIGN's thresholds (36 / 20 and 34 / 18
    past the tile origin) are written for. A build with other constants moves every case of the table with it; this test then
    says that the prose is stale."""
    assert (T.TW, T.TH, T.NT, T.HALO, T.CHALO) == (32, 16, 256, 4, 2)
    sizes = sorted(set((g.w, g.h) for g in T.THRESHOLDS))
    assert sizes == sorted([(67, 36), (68, 35), (68, 36), (69, 37), (65, 34), (66, 33), (66, 34), (67, 35)])
    assert [(g.w, g.h) for g in T.OTHER_SCALES] == [(132, 68), (136, 72), (272, 144)]
    assert [(g.w, g.h) for g in T.REDUCTIONS] == [(57344, 1), (57345, 1), (7, 74899)]
    assert sorted(T.NEGATIVE_MEAN) == sorted(g.id for g in T.FULL_GEOMETRIES)


@pytest.mark.parametrize("g", [g for g in T.GEOMETRIES if g.w * g.h <= 300 * 300], ids=lambda g: g.id)
def test_scale_shapes_are_the_restatements(g):
    from oracle import dssim_restate as D
    px = np.zeros((g.h, g.w * 3), np.uint8)
    img = D.DssimImage(px, g.w, g.h, g.w * 3, 3)
    assert [c[0]["img"].shape for c in img.scales] == [(h, w) for w, h in T.scale_chain(g.w, g.h)]


def _tile(tiles, tx, ty):
    return [t for t in tiles if t[:2] == (tx, ty)]


@pytest.mark.parametrize("g", T.GEOMETRIES, ids=[g.id for g in T.GEOMETRIES])
def test_every_claim_of_the_table_holds(g):
    chain = T.scale_chain(g.w, g.h)
    c = dict(g.claims)
    assert g.branch and g.cases
    if "scales" in c:
        assert len(chain) == c.pop("scales")
    if "size1" in c:
        assert chain[1] == c.pop("size1")
    if "last" in c:
        assert chain[-1] == c.pop("last")
    if "tiles0" in c:
        assert T.tiles(g.w, g.h) == c.pop("tiles0")
    if c.pop("narrower_than_halo", False):
        assert min(g.w, g.h) < T.HALO and len(chain) == 1
    for k, (n_scale, n_compare) in c.pop("interior", {}).items():
        assert (len(T.interior_tiles(*chain[k], T.HALO)), len(T.interior_tiles(*chain[k], T.CHALO))) == (n_scale, n_compare), k
    for name, halo, touching in (("touch_scale", T.HALO, True), ("spare_scale", T.HALO, False), ("touch_compare", T.CHALO, True),
                                 ("spare_compare", T.CHALO, False)):
        for k, (tx, ty) in c.pop(name, {}).items():
            hit = _tile(T.interior_tiles(*chain[k], halo), tx, ty)
            assert len(hit) == 1, (name, k)
            assert hit[0][2:] == ((True, True) if touching else (False, False)), (name, k, hit)
    if "grouped" in c:
        ls = T.launches(chain)
        assert [l[:2] for l in ls[:2]] == [(0, 1), (1, 1)] and len(ls) == 3 and ls[2][0] == 2 and ls[2][1] == len(chain) - 2
        assert ls[2][2] == c.pop("grouped")
    if "avg_lanes" in c:
        assert T.avg_eight_load_lanes(T.tiles(g.w, g.h)) == c.pop("avg_lanes")
    if "absdev" in c:
        blocks, trips = c.pop("absdev")
        n = g.w * g.h
        for n_cu in (1, 64, 256):
            assert T.grid_blocks(n_cu, n) == 8 * n_cu < (n + 255) // 256          # at the cap
        assert T.grid_blocks(256, n) == blocks and T.absdev_trips(n, blocks) == trips
        assert T.absdev_trips(n - 5, blocks) == trips - 1                         # five pixels fewer: one trip
    assert not c, "claims nobody checks: %r" % c


def test_no_size_but_the_touching_ones_touches_and_the_benchmark_never_does():
    """The `<=` of the interior tests is an equality on both axes at the sizes the table names for it and at no other size of the
    table; 4K and its halvings - what the benchmark and the suite's large sizes run - never reach it."""
    def touching(w, h):
        out = set()
        for k, (sw, sh) in enumerate(T.scale_chain(w, h)):
            for name, halo in (("scale", T.HALO), ("compare", T.CHALO)):
                if any(t[2] and t[3] for t in T.interior_tiles(sw, sh, halo)):
                    out.add((name, k))
        return out
    claimed = {g.id: set([("scale", k) for k in g.claims.get("touch_scale", {})] + [("compare", k) for k in g.claims.get("touch_compare", {})])
               for g in T.GEOMETRIES}
    for g in T.GEOMETRIES:
        assert touching(g.w, g.h) == claimed[g.id], g.id
    assert touching(3840, 2160) == set() and touching(1920, 1080) == set()
    assert sum(bool(v) for v in claimed.values()) == 5


def test_byte_load_forms_of_the_full_geometries():
    """RGB, RGBA wide, RGBA with stride % 8 == 4 and RGBA at allocation + 4 all occur, through the device entries, at every geometry
    that carries the full contents; the host entries upload packed rows to an aligned buffer, so an even width is always wide."""
    for g in T.FULL_GEOMETRIES:
        assert g.w % 2 == 0 and len(T.scale_chain(g.w, g.h)) >= 2           # the byte-load kernel runs only where there is a scale 1
        forms = {c.layout: c.device_form() for c in g.cases}
        assert forms["rgb"] == "rgb" and forms["rgba-wide"] == "wide" and forms["rgba-stride4"] == "bytes" and forms["rgba-base4"] == "bytes"
        by = {c.layout: c for c in g.cases}
        assert by["rgba-stride4"].stride % 8 == 4 and by["rgba-stride4"].lead == 0
        assert by["rgba-base4"].stride % 8 == 0 and by["rgba-base4"].lead == 4
        assert by["rgba-wide"].stride % 8 == 0 and by["rgba-wide"].lead == 0
        assert all(c.host_form() == ("rgb" if c.channels == 3 else "wide") for c in g.cases)
    assert T.u8_form(4, 8, 16) == "wide" and T.u8_form(4, 4, 16) == "bytes" and T.u8_form(4, 8, 12) == "bytes" and T.u8_form(3, 8, 16) == "rgb"


def test_buffers_are_poisoned_outside_the_pixels():
    for g in (T.GEOMETRIES[0], T.FULL_GEOMETRIES[0]):
        for c in g.cases:
            ref_px, _ = c.pixels()
            ref, _ = c.buffers()
            assert (ref[: c.lead] == T.POISON).all()
            rows = ref[c.lead:].reshape(c.h, c.stride)
            assert (rows[:, : c.w * c.channels] == ref_px.reshape(c.h, -1)).all() and (rows[:, c.w * c.channels:] == T.POISON).all()
            assert c.stride > c.w * c.channels


def _case(g, content):
    return next(c for c in g.cases if c.content == content)


@pytest.mark.parametrize("g", T.FULL_GEOMETRIES, ids=lambda g: g.id)
def test_inverted_blocks_drive_the_mean_ssim_below_zero(g):
    """The clamp fmax(sum / len, 0) of dssim_avg_kernel needs a scale whose mean SSIM is negative: the restatement's is, at the scales
    NEGATIVE_MEAN names and at no other."""
    import math
    _, maps, _, _ = T.reference(_case(g, "inverted"))
    negative = tuple(k for k, m in enumerate(maps) if math.fsum(m.astype(np.float64).reshape(-1)) < 0.0)
    assert negative == T.NEGATIVE_MEAN[g.id]


@pytest.mark.parametrize("g", T.FULL_GEOMETRIES, ids=lambda g: g.id)
def test_threshold_content_splits_a_packed_pair_inside_an_interior_tile(g):
    """dssim_f_pair selects per element on t > 216/24389. The gamma table puts byte 23 below it and byte 24 above; inside the region
    of a scale-0 interior tile - where the packed path runs - some pair of cells (2i, 2i + 1) of one row lies on different sides, for
    each of fx, fy and fz, in the reference frame (scale kernel) and in the modified one (hash-compare kernel)."""
    from oracle import dssim_restate as D
    lut = D.gamma_lut()
    assert lut[23] < D.EPSILON < lut[24]
    tiles = T.interior_tiles(g.w, g.h, T.HALO)
    assert tiles
    for px in _case(g, "threshold").pixels():
        assert px[..., :3].min() == 20 and px[..., :3].max() == 27
        for name, f in zip("xyz", T.lab_inputs(px)):
            above = f > D.EPSILON
            hits = 0
            for tx, ty, _, _ in tiles:
                x0, y0 = tx * T.TW - T.HALO, ty * T.TH - T.HALO
                assert x0 % 2 == 0
                region = above[y0: y0 + T.TH + 2 * T.HALO, x0: x0 + T.TW + 2 * T.HALO]
                hits += int((region[:, 0::2] != region[:, 1::2]).sum())
            assert hits > 0, name


@pytest.mark.parametrize("g", T.FULL_GEOMETRIES, ids=lambda g: g.id)
def test_translucent_content_meets_every_pattern_bit_and_both_alpha_branches(g):
    """Alpha is drawn from {0, 1, 254, 255}. Inside the region of a scale-0 interior tile, pixels with a != 1 (the ones
    dssim_linear_px hands to dssim_pattern) meet each of the bits 8, 16, 32 of (x + 11) ^ (y + 11) set and clear; at scale 1 some
    2 x 2 block averages to alpha exactly 1.0 (pattern skipped) and some to less."""
    from oracle import dssim_restate as D
    tiles = T.interior_tiles(g.w, g.h, T.HALO)
    assert tiles
    for content in ("translucent", "translucent-black"):
        c = _case(g, content)
        assert c.pattern == (content == "translucent")
        for px in c.pixels():
            alpha = px[..., 3]
            assert set(np.unique(alpha)) == {0, 1, 254, 255}
            yy, xx = np.mgrid[0: g.h, 0: g.w]
            n = (xx + 11) ^ (yy + 11)
            inside = np.zeros((g.h, g.w), bool)
            for tx, ty, _, _ in tiles:
                x0, y0 = tx * T.TW - T.HALO, ty * T.TH - T.HALO
                inside[y0: y0 + T.TH + 2 * T.HALO, x0: x0 + T.TW + 2 * T.HALO] = True
            sel = inside & (alpha != 255)
            for bit in (8, 16, 32):
                assert (n[sel] & bit).any() and (~n[sel] & bit).any(), bit
            lin1 = D.downsample(D.to_linear(px.reshape(-1), g.w, g.h, g.w * 4, 4))
            assert (lin1[..., 3] == 1.0).any() and (lin1[..., 3] < 1.0).any()
