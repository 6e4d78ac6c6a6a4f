"""GPU tests for the memory policy of hsvfilter's flat kernels (MI355_FLAG_HSV_NT): 0 plain loads and stores, 1 both with the
non-temporal hint, 2 plain loads and write-through stores that stay in the Infinity Cache (hsv_kernels.hip: hsv_store_through, one
global_store_dwordx4 with sc0 sc1 per lane). The arithmetic is the same under all three, so the bar is `==` on every byte - the
frames and 64 sentinel bytes on either side of them - against the C oracle, through the context's entry
(hsvfilter_flat_kernel), the group's filter queue (hsvfilter_jobs_kernel) and the group's chain batches
(hsvfilter_flat_multi_kernel), and for the hand-over to the colorlut launch behind it on the same stream.

Shapes (width, height, frames): one vector in one lane; 65 vectors, a second wave with one lane; a flat batch of several blocks;
8738 vectors on 18 blocks, a grid-stride tail that is no multiple of the block."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((4, 1, 1), (260, 1, 1), (64, 16, 3), (1028, 17, 2))
FMTS = ("RGBA", "xRGB")
GUARD = 64
GENERIC = (1.0e7, 1.25, -0.05, 0.8, 0.1)     # beyond 2^22: the GENERIC variant (fmodf of a large operand)


def settings_of(name):
    from mi355fx import synth
    return GENERIC if name == "generic" else synth.HSV_SETTINGS[name]


@functools.lru_cache(maxsize=None)
def case(w, h, n, fmt, name):
    """(arena, expected arena) for n frames of w x h back to back between two guards; computed once, read-only."""
    from mi355fx import FMT_LAYOUT
    from oracle import oracle as O
    ps, first, bgr = FMT_LAYOUT[fmt]
    rng = np.random.default_rng(w * 131 + h * 17 + n)
    nbytes = w * h * n * ps
    arena = ((np.arange(nbytes + 2 * GUARD, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
    arena[GUARD:GUARD + nbytes] = rng.integers(0, 256, nbytes, dtype=np.uint8)
    exp = arena.copy()
    O.hsvfilter(exp[GUARD:GUARD + nbytes], w, w * ps, ps, first, bool(bgr), settings_of(name))
    assert (exp != arena).any() and (exp[:GUARD] == arena[:GUARD]).all() and (exp[-GUARD:] == arena[-GUARD:]).all()
    arena.setflags(write=False)
    exp.setflags(write=False)
    return arena, exp


def upload(ctx, arena):
    d = ctx.alloc(arena.nbytes)
    assert d % 16 == 0
    ctx.h2d(d, arena)
    return d


def download(ctx, d, nbytes):
    out = np.zeros(nbytes, np.uint8)
    ctx.synchronize()
    ctx.d2h(out, d)
    return out


@pytest.mark.parametrize("name", ["hue90", "generic"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_context_entry_equals_the_oracle(ctx, oracle, policy, fmt, name):
    import mi355fx
    ctx.set_flag(mi355fx.FLAG_HSV_NT, policy)
    for w, h, n in SHAPES:
        arena, exp = case(w, h, n, fmt, name)
        d = upload(ctx, arena)
        try:
            ctx.hsvfilter_frames_device(d + GUARD, n, w * h * 4, w, h, w * 4, fmt, settings_of(name))
            got = download(ctx, d, arena.nbytes)
        finally:
            ctx.free(d)
        assert (got == exp).all(), (policy, fmt, name, (w, h, n), np.flatnonzero(got != exp)[:8])


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_group_queue_equals_the_context(ctx, oracle, policy, members):
    """Every member one frame of the shape, each in an arena of its own; the lone entry on a copy."""
    import mi355fx
    ctx.set_flag(mi355fx.FLAG_HSV_NT, policy)
    g = mi355fx.Group(0)
    try:
        for w, h, _ in SHAPES:
            for fmt in FMTS:
                for name in ("hue90", "generic"):
                    arena, exp = case(w, h, 1, fmt, name)
                    st = settings_of(name)
                    dg = [upload(ctx, arena) for _ in range(members)]
                    dl = upload(ctx, arena)
                    try:
                        tickets = [g.submit_hsvfilter(ctx, d + GUARD, w, h, w * 4, fmt, st) for d in dg]
                        for t in tickets:
                            g.wait_hsvfilter(t)
                        ctx.hsvfilter_frames_device(dl + GUARD, 1, 0, w, h, w * 4, fmt, st)
                        lone = download(ctx, dl, arena.nbytes)
                        got = [download(ctx, d, arena.nbytes) for d in dg]
                    finally:
                        for d in dg + [dl]:
                            ctx.free(d)
                    assert (lone == exp).all(), (policy, (w, h), fmt, name)
                    for m, out in enumerate(got):
                        assert (out == lone).all(), (policy, members, m, (w, h), fmt, name, np.flatnonzero(out != lone)[:8])
    finally:
        g.close()


def lut_and_expected(oracle, synth, w, h, frames_rgba, st):
    """frames through the oracle's hsvfilter then its colorlut: (parsed LUT for colorlut_load, filtered frames, mapped frames)"""
    from mi355fx.cube import parse_cube
    text = synth.cube_text_3d(17)
    ocube = oracle.Cube.parse(text)
    mid = frames_rgba.copy()
    out = np.zeros_like(mid)
    for f in range(mid.shape[0]):
        oracle.hsvfilter(mid[f], w, w * 4, 4, 0, False, st)
        oracle.colorlut_rgba8(ocube, mid[f], w * 4, out[f], w * 4, w, h)
    return parse_cube(text), mid, out


def test_hand_over_to_colorlut_on_the_same_stream(ctx, oracle, synth):
    """Policy 2, then colorlut on the same buffer and stream with nothing in between: a write-through store is still a store of
    the launch that issued it, complete before the next launch's loads."""
    import mi355fx
    w, h, n = 64, 16, 3
    st = synth.HSV_SETTINGS["hue90"]
    arena, _ = case(w, h, n, "RGBA", "hue90")
    nbytes = w * h * 4 * n
    lut, mid, exp = lut_and_expected(oracle, synth, w, h, arena[GUARD:GUARD + nbytes].reshape(n, -1), st)
    ctx.set_flag(mi355fx.FLAG_HSV_NT, 2)
    ctx.colorlut_load(lut.is3d, lut.size, lut.table, lut.domain_scale, lut.domain_offset)
    d_src, d_dst = upload(ctx, arena), upload(ctx, np.full(arena.nbytes, 0x5a, np.uint8))
    try:
        pitch = w * h * 4
        ctx.hsvfilter_frames_device(d_src + GUARD, n, pitch, w, h, w * 4, "RGBA", st)
        ctx.colorlut_frames_device(d_src + GUARD, pitch, w * 4, d_dst + GUARD, pitch, w * 4, n, w, h, "RGBA")
        got_mid, got = download(ctx, d_src, arena.nbytes), download(ctx, d_dst, arena.nbytes)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    assert (got_mid[GUARD:-GUARD] == mid.reshape(-1)).all()
    assert (got[GUARD:-GUARD] == exp.reshape(-1)).all(), np.flatnonzero(got[GUARD:-GUARD] != exp.reshape(-1))[:8]
    assert (got[:GUARD] == 0x5a).all() and (got[-GUARD:] == 0x5a).all()


@pytest.mark.parametrize("policy", [0, 2])
def test_chain_batches_take_the_members_policy(oracle, synth, policy):
    """Three streams' frames as one chain batch (hsvfilter_flat_multi_kernel, then the multi-frame table kernel): 132 vectors per
    frame, so a frame's third wave is partly filled (the batched colorlut kernel takes widths that are multiples of 4, from 128)."""
    import mi355fx
    w, h = 132, 4
    st = synth.HSV_SETTINGS["hue90"]
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (3, w * h * 4), dtype=np.uint8)
    lut, mid, exp = lut_and_expected(oracle, synth, w, h, frames, st)
    ctxs = [mi355fx.Context(0) for _ in range(3)]
    g = mi355fx.Group(0)
    bufs = []
    try:
        for c in ctxs:
            c.set_flag(mi355fx.FLAG_HSV_NT, policy)
            c.colorlut_load(lut.is3d, lut.size, lut.table, lut.domain_scale, lut.domain_offset)
        for c, f in zip(ctxs, frames):
            bufs.append((c, upload(c, f), upload(c, np.zeros_like(f))))
        tickets = [g.submit_chain(c, ds, dd, w, h, w * 4, "RGBA", st) for c, ds, dd in bufs]
        for t in tickets:
            g.wait(t)
        assert tuple(g.stats())[:3] == (3, 1, 0)      # one batched launch pair carried all three
        for i, (c, ds, dd) in enumerate(bufs):
            assert (download(c, ds, frames[i].nbytes) == mid[i]).all(), (policy, i)
            assert (download(c, dd, frames[i].nbytes) == exp[i]).all(), (policy, i)
    finally:
        g.close()
        for c, ds, dd in bufs:
            c.free(ds)
            c.free(dd)
        for c in ctxs:
            c.close()
