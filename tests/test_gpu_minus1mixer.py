"""minus1mixer / audiomultimixer on the GPU, one mixer on one context (csrc/mixer.hip): every output sample compared BY BITS with the
restatement of aggregate_one_buffer + split_output_buf (tests/minus1mixer_restate.py); an F32 sample that is NaN there has to be NaN
here. Shapes sit around the kernel's frame tile T, its 16-channel groups, one 64-candidate ballot word and the limits."""
import ctypes as C

import numpy as np
import pytest

import minus1mixer_cases as M
import minus1mixer_restate as R
import mi355fx

pytestmark = pytest.mark.gpu

F32, S16 = R.F32, R.S16
T = mi355fx.MIXER_FRAME_TILE
FRAMES = [1, 7, T - 1, T, T + 1, 480, 2 * T + 3]
NS = [1, 2, 3, 5, 63, 64, 65, 256]


def run_host(ctx, case, setup=True):
    if setup:
        ctx.mixer_setup(case.contrib)
    bufs = case.buffers()
    ctx.mixer_process(*case.call(bufs), case.frames)
    return bufs


def run_device(ctx, case, setup=True):
    """the same call on device memory; every segment starts 4 (F32) or 2 (S16) bytes into its allocation: aligned to its sample, not
    to 16 bytes"""
    if setup:
        ctx.mixer_setup(case.contrib)
    held, segs, outs = [], [], []
    try:
        for inp, data, off in case.segments:
            skew = data.itemsize
            p = ctx.alloc(data.nbytes + 32)
            held.append(p)
            if data.size:
                ctx.h2d(p + skew, data)
            segs.append((inp, (p + skew, R.fmt_of(data), data.size), off))
        bufs = case.buffers()
        for b, (fmt, off, nch) in zip(bufs, case.outputs):
            p = ctx.alloc(b.nbytes + 32)
            held.append(p)
            if b.size:
                ctx.h2d(p, b)
            outs.append(((p, fmt), off, nch))
        ctx.synchronize()
        ctx.mixer_process_device(segs, outs, case.frames)
        ctx.synchronize()
        for b, (pf, _, _) in zip(bufs, outs):
            if b.size:
                ctx.d2h(b, pf[0])
        return bufs
    finally:
        for p in held:
            ctx.free(p)


# ---------------------------------------------------------------- known answers

@pytest.mark.parametrize("fmt", [F32, S16], ids=["F32", "S16"])
def test_reference_vectors_1_10_100(ctx, fmt):
    case = M.reference_vectors(fmt, fmt)
    ctx.mixer_setup_minus1(3)
    got = run_host(ctx, case, setup=False)
    for out, want in zip(got, (110, 101, 11)):
        assert (out == want).all()
    M.assert_same(got, case)


# ---------------------------------------------------------------- random sweep, minus-1 matrix

@pytest.mark.parametrize("n", NS)
def test_minus1_random_sweep(ctx, n):
    ctx.mixer_setup_minus1(n)
    for k, frames in enumerate(FRAMES):
        case = M.random_minus1(1000 * n + k, n, frames)
        M.assert_same(run_host(ctx, case, setup=False), case)


# ---------------------------------------------------------------- general matrices

@pytest.mark.parametrize("n_in,n_out,frames", [(3, 2, 480), (5, 7, T + 1), (65, 33, 2 * T + 3), (2, 256, T - 1), (256, 17, 7)])
def test_general_matrices(ctx, n_in, n_out, frames):
    case = M.random_general(n_in * 1000 + n_out, n_in, n_out, frames)
    got = run_host(ctx, case)
    M.assert_same(got, case)
    assert not got[0].any() and not got[1].view(np.uint32).any()   # the channel nobody feeds


# ---------------------------------------------------------------- the order of the segments is the order of the additions

@pytest.mark.parametrize("n", [3, 65])
def test_segments_are_added_in_array_order(ctx, n):
    frames = T + 1
    vals = np.ones(n, np.float32)
    vals[0], vals[n - 1] = 1e8, -1e8            # the large pair at rows 0 and n - 1 (64: the second ballot word)
    segs = [(i, np.full(frames, vals[i], np.float32), 0) for i in range(n)]
    in_order = M.Case(np.ones((n, 1), bool), segs, [(F32, 0, 1)], frames, "order: as numbered")
    pair_first = M.Case(np.ones((n, 1), bool), [segs[0], segs[n - 1]] + segs[1:n - 1], [(F32, 0, 1)], frames, "order: pair first")
    a, b = run_host(ctx, in_order)[0], run_host(ctx, pair_first, setup=False)[0]
    M.assert_same([a], in_order)
    M.assert_same([b], pair_first)
    assert (a == 0.0).all() and (b == np.float32(n - 2)).all()


# ---------------------------------------------------------------- segments

def _segment_case():
    rng = np.random.default_rng(77)
    frames = 2 * T + 3
    s = lambda fmt, n: M.samples(rng, fmt, n)
    segs = [
        (0, s(F32, 20), 5),                                   # starts after frame 0, ends before `frames`
        (1, s(S16, 30), 0), (1, s(S16, T - 30), 30),          # back to back, meeting inside a tile
        (1, s(F32, T + 3), T),                                # ... and exactly at a tile edge (another format, too)
        (3, s(F32, 0), 0),                                    # no frames
        (3, s(S16, frames), 0),
        (0, s(S16, 9), 2 * T - 6),                            # a second buffer of input 0, across the last tile edge
    ]                                                         # input 2 sends nothing
    outs = [(o % 2, o, 1) for o in range(4)]
    return M.Case(R.minus1(4), segs, outs, frames, "segments")


def test_segment_geometry_host_and_device(ctx):
    case = _segment_case()
    M.assert_same(run_host(ctx, case), case)
    M.assert_same(run_device(ctx, case, setup=False), case)


def test_no_segment_at_all_is_silence(ctx):
    case = M.Case(R.minus1(3), [], [(F32, 0, 1), (S16, 1, 1), (F32, 2, 1)], T + 1, "no segments")
    got = run_host(ctx, case)
    assert all(not g.view(np.uint8).any() for g in got)
    M.assert_same(got, case)


def test_1024_segments(ctx):
    rng = np.random.default_rng(1024)
    frames = T + 1
    segs = []
    for _ in range(1024):
        n = int(rng.integers(0, 4))
        segs.append((int(rng.integers(0, 4)), M.samples(rng, int(rng.integers(0, 2)), n), int(rng.integers(0, frames - n + 1))))
    case = M.Case(R.minus1(4), segs, [(o % 2, o, 1) for o in range(4)], frames, "1024 segments")
    M.assert_same(run_host(ctx, case), case)


def test_frames_zero_is_fine(ctx):
    ctx.mixer_setup_minus1(2)
    ctx.mixer_process([(0, np.zeros(0, np.float32), 0)], [(np.zeros(0, np.float32), 0, 1)], 0)


# ---------------------------------------------------------------- special values at the edges of a tile (= lanes 0 and 63)

@pytest.mark.parametrize("name,values,f32_bits,s16", M.SPECIALS, ids=[s[0] for s in M.SPECIALS])
def test_special_values_at_tile_edges(ctx, name, values, f32_bits, s16):
    at = (0, T - 1, T, 2 * T - 1)
    filler = np.arange(1, len(values) + 1).astype(values.dtype)
    case = M.special_case(values, frames=2 * T, at=at, filler=filler)
    f, s = run_host(ctx, case)
    M.assert_same([f, s], case)
    for i in at:
        if f32_bits is None:
            assert np.isnan(f[i])
        else:
            assert int(f.view(np.uint32)[i]) == f32_bits, (i, hex(int(f.view(np.uint32)[i])))
        assert int(s[i]) == s16, i


# ---------------------------------------------------------------- setup and paths

def test_setup_again_between_intervals_leaves_no_stale_matrix(ctx):
    for k, n in enumerate((3, 5, 2)):
        ctx.mixer_setup_minus1(n)
        case = M.random_minus1(40 + k, n, T + 1)
        M.assert_same(run_host(ctx, case, setup=False), case)
    ctx.mixer_reset()
    with pytest.raises(mi355fx.Mi355Error) as e:
        run_host(ctx, case, setup=False)
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED


@pytest.mark.parametrize("n,frames", [(5, 480), (65, T + 1)])
def test_host_buffers_equal_device_buffers(ctx, n, frames):
    case = M.random_minus1(900 + n, n, frames)
    host, dev = run_host(ctx, case), run_device(ctx, case, setup=False)
    for h, d in zip(host, dev):
        assert h.tobytes() == d.tobytes()
    M.assert_same(dev, case)


# ---------------------------------------------------------------- errors: an argument check that returns before anything is launched or written

def _raw(ctx, segs, outs, frames, device=False):
    sa = (mi355fx.MixerSegment * max(len(segs), 1))(*[mi355fx.MixerSegment(*s) for s in segs])
    oa = (mi355fx.MixerOutput * max(len(outs), 1))(*[mi355fx.MixerOutput(*o) for o in outs])
    fn = ctx.L.mi355_mixer_process_device if device else ctx.L.mi355_mixer_process
    return fn(ctx.h, sa, len(segs), oa, len(outs), frames)


def test_documented_errors_write_nothing(ctx):
    frames = 8
    x = np.ones(frames, np.float32)
    out = M.Case(R.minus1(3), [], [(F32, 0, 1), (S16, 2, 1)], frames).buffers()
    xp, o0, o1 = x.ctypes.data, out[0].ctypes.data, out[1].ctypes.data
    good_seg, good_outs = (xp, 0, 0, 0, frames), [(o0, 0, 0, 1), (o1, 1, 2, 1)]
    assert _raw(ctx, [good_seg], good_outs, frames) == mi355fx.ERR_NOT_CONFIGURED
    assert _raw(ctx, [good_seg], good_outs, frames, device=True) == mi355fx.ERR_NOT_CONFIGURED
    ctx.mixer_setup_minus1(3)
    bad = {
        "input >= n_inputs": ([(xp, 3, 0, 0, frames)], good_outs),
        "segment format": ([(xp, 0, 2, 0, frames)], good_outs),
        "segment past the interval": ([(xp, 0, 0, 1, frames)], good_outs),
        "offset past the interval": ([(xp, 0, 0, frames + 1, 0)], good_outs),
        "null segment data": ([(None, 0, 0, 0, frames)], good_outs),
        "output format": ([good_seg], [(o0, 7, 0, 1), good_outs[1]]),
        "channels past n_out": ([good_seg], [good_outs[0], (o1, 1, 2, 2)]),
        "channel offset past n_out": ([good_seg], [good_outs[0], (o1, 1, 3, 1)]),
        "no channels": ([good_seg], [good_outs[0], (o1, 1, 2, 0)]),
        "null output data": ([good_seg], [good_outs[0], (None, 1, 2, 1)]),
    }
    for why, (segs, outs) in bad.items():
        for device in (False, True):   # (the device form checks before it touches a pointer, so host addresses do for it here)
            assert _raw(ctx, [good_seg] + segs, outs, frames, device) == mi355fx.ERR_INVALID_ARG, why
    # the device form loads samples by their type: a pointer that is not aligned to it is refused (the host form packs, and takes any)
    for segs, outs in (([(xp + 2, 0, 0, 0, frames - 1)], good_outs), ([(xp + 1, 0, 1, 0, frames - 1)], good_outs),
                       ([good_seg], [(o0 + 2, 0, 0, 1), good_outs[1]]), ([good_seg], [good_outs[0], (o1 + 1, 1, 2, 1)])):
        assert _raw(ctx, segs, outs, frames - 1, device=True) == mi355fx.ERR_INVALID_ARG
    assert M.untouched(out)
    assert _raw(ctx, [good_seg], good_outs, frames) == 0 and not M.untouched(out)   # the same call without the flaw goes through


def test_limits_are_unsupported(ctx):
    for n_in, n_out in ((257, 3), (3, 257)):
        m = np.ones((n_in, n_out), np.uint8)
        assert ctx.L.mi355_mixer_setup(ctx.h, n_in, n_out, m.ctypes.data) == mi355fx.ERR_UNSUPPORTED
    assert ctx.L.mi355_mixer_setup_minus1(ctx.h, 257) == mi355fx.ERR_UNSUPPORTED
    assert ctx.L.mi355_mixer_setup_minus1(ctx.h, 0) == mi355fx.ERR_INVALID_ARG
    assert ctx.L.mi355_mixer_setup(ctx.h, 2, 2, None) == mi355fx.ERR_INVALID_ARG
    ctx.mixer_setup_minus1(2)
    out = M.Case(R.minus1(2), [], [(F32, 0, 1)], 4).buffers()
    x = np.ones(4, np.float32)
    seg = (x.ctypes.data, 0, 0, 0, 4)
    assert _raw(ctx, [seg] * 1025, [(out[0].ctypes.data, 0, 0, 1)], 4) == mi355fx.ERR_UNSUPPORTED
    assert _raw(ctx, [seg], [(out[0].ctypes.data, 0, 0, 1)], (1 << 20) + 1, device=True) == mi355fx.ERR_UNSUPPORTED
    assert _raw(ctx, [seg], [(out[0].ctypes.data, 0, 0, 1)] * 1025, 4) == mi355fx.ERR_UNSUPPORTED
    assert M.untouched(out)
    assert _raw(ctx, [seg] * 1024, [(out[0].ctypes.data, 0, 1, 1)], 4) == 0 and (out[0] == 1024.0).all()
