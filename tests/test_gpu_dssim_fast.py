"""GPU tests of the Dssim fast form (MI355_FLAG_DSSIM_FAST = 1: gst-plugins-rs_amd/csrc/dssim_fast.hip) and of the public pairs entry
points. The fast form is held to the f64 evaluation of oracle/dssim_restate.py (tests/dssim_f64.py: the oracle's own text with
F = float64), within the exact form's own f32 rounding noise. Tolerances are computed here from the oracle, never from the device:
over the suite at a size, N_d / N_map = max |f32 restatement - f64 evaluation| of the score / of a map pixel; the device must stay
within 2 x N_d of the f64 score and within 2 x N_map of every f64 map pixel (an unfused separable f32 evaluation sits at 1.4 / 1.3;
an indexing, halo or border mistake moves a map pixel by 1e-2 or more). Each test prints N_d, N_map and the device's worst ratios."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dssim_f64 as Y  # noqa: E402

pytestmark = pytest.mark.gpu

TW, TH = 32, 16   # the pair kernel's tile
_yardstick = {}


def _reference(w, h, channels, stride, pattern):
    """(cases, N_d, N_map, [(d64, maps64)]) of a size: computed once, shared, never changed."""
    key = (w, h, channels, stride, pattern)
    if key not in _yardstick:
        cases = Y.suite(w, h, channels, stride)
        _yardstick[key] = (cases,) + Y.noise(cases, w, h, pattern)
    return _yardstick[key]


def _upload(c, a):
    d = c.alloc(a.nbytes)
    c.h2d(d, a.reshape(-1))
    return d


def _fmt(ch):
    return "RGBA" if ch == 4 else "RGB"


def _scales(w, h):
    out = [(w, h)]
    while len(out) < 5 and w >= 8 and h >= 8:
        w, h = w // 2, h // 2
        out.append((w, h))
    return out


def _map(c, da, db, st, w, h, ch, k, mw, mh):
    """The SSIM map of scale k through a sentinel-filled buffer: all of the map is written, nothing behind it."""
    buf = np.full(mw * mh + 64, np.nan, np.float32)
    c.dssim_pair_map_device(da, db, st, w, h, _fmt(ch), k, buf)
    assert np.isnan(buf[mw * mh:]).all(), "written past the map"
    assert np.isfinite(buf[:mw * mh]).all(), "map pixels left unwritten"
    return buf[:mw * mh].reshape(mh, mw).astype(np.float64)


SIZES = [(8, 8, None, None, True), (37, 19, 4, None, True), (37, 19, 4, None, False), (64, 33, 3, 64 * 3 + 5, True), (128, 96, None, None, True),
         (322, 246, None, None, True)]
SIZES += [(TW + dx, TH + dy, None, None, True) for dx, dy in ((-2, -2), (-1, -1), (1, 1), (2, 2), (-2, 1), (-1, 2), (1, -2), (2, -1))]


@pytest.mark.parametrize("w,h,channels,stride,pattern", SIZES)
def test_fast_maps_and_scores_within_twice_the_exact_forms_f32_noise(ctx, w, h, channels, stride, pattern):
    import mi355fx
    cases, n_d, n_map, ref64 = _reference(w, h, channels, stride, pattern)
    assert n_d > 0.0 and n_map > 0.0
    ctx.set_flag(mi355fx.FLAG_DSSIM_FAST, 1)
    ctx.set_flag(mi355fx.FLAG_DSSIM_TRANSLUCENT, 0 if pattern else 1)
    worst_d = worst_map = 0.0
    bufs = []
    try:
        # scores: the cases of one format in one call (several pairs per call)
        for ch in (3, 4):
            idx = [i for i, cs in enumerate(cases) if cs[4] == ch]
            if not idx:
                continue
            pairs = [(_upload(ctx, cases[i][1]), _upload(ctx, cases[i][2])) for i in idx]
            bufs += [d for p in pairs for d in p]
            st = cases[idx[0]][3]
            got = ctx.dssim_compare_pairs_device([p[0] for p in pairs], [p[1] for p in pairs], st, w, h, _fmt(ch))
            for i, (da, db), g in zip(idx, pairs, got):
                d64, m64 = ref64[i]
                worst_d = max(worst_d, abs(g - d64) / n_d)
                assert len(m64) == len(_scales(w, h))
                for k, (mw, mh) in enumerate(_scales(w, h)):
                    m = _map(ctx, da, db, st, w, h, ch, k, mw, mh)
                    worst_map = max(worst_map, float(np.abs(m - m64[k]).max()) / n_map)
        print("dssim fast %dx%d ch=%s pattern=%s: N_d %.3e N_map %.3e device/N: score %.3f map %.3f" % (w, h, channels, pattern, n_d, n_map, worst_d, worst_map))
        assert worst_map <= 2.0, (worst_map, n_map)
        assert worst_d <= 2.0, (worst_d, n_d)
    finally:
        for d in bufs:
            ctx.free(d)


@pytest.mark.parametrize("w,h,kind", [(8, 8, "noise"), (37, 19, "translucent"), (128, 96, "noise"), (322, 246, "flat"), (3840, 2160, "red")])
def test_fast_identical_frames_give_exactly_zero(ctx, w, h, kind):
    """The reference's only pinned fact (videocompare.rs:145-182: red against red, distance <= 0.0), by construction in the fast form."""
    import mi355fx
    rng = np.random.default_rng(w + h)
    if kind == "red":
        f = np.zeros((h, w, 4), np.uint8); f[..., 0] = 255; f[..., 3] = 255
    elif kind == "flat":
        f = np.full((h, w, 4), 200, np.uint8); f[..., 3] = 255
    else:
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        f[..., 3] = np.where(rng.random((h, w)) < 0.2, rng.integers(0, 255, (h, w)), 255) if kind == "translucent" else 255
    ctx.set_flag(mi355fx.FLAG_DSSIM_FAST, 1)
    da, db = _upload(ctx, f), _upload(ctx, f.copy())
    try:
        got = ctx.dssim_compare_pairs_device([da, da], [db, da], w * 4, w, h)
        assert got[0] == 0.0 and got[1] == 0.0, got
        if w <= 322:
            for k, (mw, mh) in enumerate(_scales(w, h)):
                assert (_map(ctx, da, db, w * 4, w, h, 4, k, mw, mh) == 1.0).all()
    finally:
        ctx.free(da); ctx.free(db)


def _pair_frames(w, h, ch, amps=(3, 25)):
    rng = np.random.default_rng(w * 3 + h + ch)
    ref = rng.integers(0, 256, (h, w * ch), dtype=np.uint8)
    mods = [np.clip(ref.astype(int) + rng.integers(-a, a + 1, ref.shape), 0, 255).astype(np.uint8) for a in amps]
    if ch == 4:
        for f in [ref] + mods:
            f[:, 3::4] = 255
    return ref, mods


@pytest.mark.parametrize("w,h,ch", [(128, 96, 4), (37, 19, 3)])
def test_flag_zero_pairs_are_the_exact_path_bit_for_bit(ctx, w, h, ch):
    ref, mods = _pair_frames(w, h, ch)
    dr, dm = _upload(ctx, ref), [_upload(ctx, m) for m in mods]
    try:
        got = ctx.dssim_compare_pairs_device([dr] * len(dm), dm, w * ch, w, h, _fmt(ch))
        img = ctx.dssim_create_image_device(dr, w * ch, w, h, _fmt(ch))
        exp = ctx.dssim_compare_frames_device(img, dm, w * ch, w, h, _fmt(ch))
        assert got == exp and all(v > 0.0 for v in got)
        assert ctx.dssim_compare_pairs([ref] * len(mods), mods, w * ch, w, h, _fmt(ch)) == exp   # host pointers: the same values
        for m, e in zip(mods, exp):
            other = ctx.dssim_create_image(m, w * ch, w, h, _fmt(ch))
            assert ctx.dssim_compare(img, other) == pytest.approx(e, rel=1e-9, abs=1e-13)
            ctx.dssim_free_image(other)
        # the exact form's map through the diagnostic is the restatement's, bit for bit
        from oracle import dssim_restate as D
        _, maps = D.compare(D.DssimImage(ref, w, h, w * ch, ch), D.DssimImage(mods[0], w, h, w * ch, ch), return_maps=True)
        for k, (mw, mh) in enumerate(_scales(w, h)):
            assert (_map(ctx, dr, dm[0], w * ch, w, h, ch, k, mw, mh).astype(np.float32) == maps[k]).all()
        ctx.dssim_free_image(img)
    finally:
        for d in [dr] + dm:
            ctx.free(d)


def test_flag_is_sticky_image_handles_stay_exact_and_bad_arguments_are_refused(ctx):
    import mi355fx
    w, h, ch = 64, 40, 4
    ref, mods = _pair_frames(w, h, ch)
    dr, dm = _upload(ctx, ref), [_upload(ctx, m) for m in mods]
    F = mi355fx.FLAG_DSSIM_FAST
    try:
        call = lambda: ctx.dssim_compare_pairs_device([dr] * len(dm), dm, w * ch, w, h)
        exact = call()
        img = ctx.dssim_create_image_device(dr, w * ch, w, h)
        ctx.set_flag(F, 1)
        fast = call()
        assert fast != exact and np.allclose(fast, exact, rtol=0, atol=1e-3)
        assert ctx.dssim_compare_frames_device(img, dm, w * ch, w, h) == exact       # an image handle is the exact form's object
        assert ctx.dssim_compare_pairs([ref] * len(mods), mods, w * ch, w, h) == fast
        with pytest.raises(mi355fx.Mi355Error):
            ctx.set_flag(F, 2)
        with pytest.raises(mi355fx.Mi355Error):
            ctx.set_flag(F, -1)
        assert call() == fast                                                        # a refused value changes nothing
        ctx.set_flag(F, 0)
        assert call() == exact
        ctx.set_flag(F, 1)
        assert call() == fast
        ctx.dssim_free_image(img)
        for flag in (0, 1):
            ctx.set_flag(F, flag)
            with pytest.raises(mi355fx.Mi355Error):
                ctx.dssim_compare_pairs_device([dr], [dm[0]], w * ch - 1, w, h)      # rows shorter than the width
            with pytest.raises(mi355fx.Mi355Error):
                ctx.dssim_compare_pairs_device([dr] * 65, [dm[0]] * 65, w * ch, w, h)
            with pytest.raises(mi355fx.Mi355Error):
                ctx.dssim_compare_pairs_device([dr], [dm[0]], w * ch, w, h, "BGRx")
            with pytest.raises(mi355fx.Mi355Error):
                ctx.dssim_pair_map_device(dr, dm[0], w * ch, w, h, "RGBA", 5)
            with pytest.raises(mi355fx.Mi355Error):
                ctx.dssim_pair_map_device(dr, dm[0], w * ch, 16, 6, "RGBA", 1)         # 16 x 6 has one scale
            with pytest.raises(ValueError):
                ctx.dssim_compare_pairs_device([dr, dr], [dm[0]], w * ch, w, h)
            assert ctx.dssim_compare_pairs_device([], [], w * ch, w, h) == []
            # the scores land in their n doubles and nowhere else
            n = len(dm)
            out = (C.c_double * (n + 8))(*([-7.0] * (n + 8)))
            pr, pf = (C.c_void_p * n)(*[int(dr)] * n), (C.c_void_p * n)(*[int(d) for d in dm])
            assert ctx.L.mi355_dssim_compare_pairs_device(ctx.h, pr, pf, n, w * ch, w, h, mi355fx.FMT["RGBA"], out) == 0
            assert list(out)[:n] == (fast if flag else exact) and list(out)[n:] == [-7.0] * 8
    finally:
        for d in [dr] + dm:
            ctx.free(d)


def test_group_batches_never_mix_the_two_forms(mi355lib):
    """Members of a fast and of an exact context submit pairs of one geometry in the same interval: each gets what its own context's
    dssim_compare_pairs_device gives, and the two forms run as separate launch sequences."""
    import mi355fx
    w, h, ch = 96, 64, 4
    ref, mods = _pair_frames(w, h, ch, amps=(2, 9, 30, 70))
    ctxs = [mi355fx.Context(0) for _ in range(4)]
    g = mi355fx.Group(0)
    try:
        for c in ctxs[:2]:
            c.set_flag(mi355fx.FLAG_DSSIM_FAST, 1)
        pairs = [(_upload(c, ref), _upload(c, m)) for c, m in zip(ctxs, mods)]
        own = [c.dssim_compare_pairs_device([a], [b], w * ch, w, h)[0] for c, (a, b) in zip(ctxs, pairs)]
        plain = mi355fx.Context(0)
        try:
            d = [_upload(plain, ref)] + [_upload(plain, m) for m in mods]
            exact = plain.dssim_compare_pairs_device([d[0]] * 4, d[1:], w * ch, w, h)
            for x in d:
                plain.free(x)
        finally:
            plain.close()
        assert own[2:] == exact[2:] and all(o != e for o, e in zip(own[:2], exact[:2]))
        tk = [g.submit_compare(ctxs[s], pairs[s][0], pairs[s][1], w * ch, w, h, "RGBA", 5) for s in (2, 0, 3, 1)]
        got = dict(zip((2, 0, 3, 1), [g.wait_compare(t)[0] for t in tk]))
        assert [got[s] for s in range(4)] == own
        st = g.compare_stats()
        assert st[0] == 4 and st[1] == 2 and st[2] == 2, st      # four pairs, two launch sequences of two
        for c, (a, b) in zip(ctxs, pairs):
            c.free(a); c.free(b)
    finally:
        g.close()
        for c in ctxs:
            c.close()
