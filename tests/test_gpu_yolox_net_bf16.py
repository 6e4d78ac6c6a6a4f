"""The BF16 precision of yoloxinference's network on the GPU (mi355_yolox_net_set_precision, yolox_conv_mfma_kernel)
against tests/yolox_net_bf16.py.

Single ops go through mi355_selftest_yolox_net_op_bf16_device: 2 frames, written at a nonzero channel offset into a wider buffer whose
other channels hold a sentinel that must survive, under both tile shapes of the kernel and under the forward's own choice - the same
bytes. Spatial sizes 1 x 1, 2 x 2, 5 x 7 and 9 x 9 (81 pixels: the widest pixel tile, 64, and 17 more - no multiple of 16); channel
counts 1 .. 65 (33 crosses a reduction step of 32 at k = 1, 4 x 9 = 36 at k = 3, 65 a 64-channel tile).
1. a permutation as a 1 x 1 convolution, 2. one tap per output channel at k = 3, 3. small integers: bit for bit whatever the matrix
unit's order is. 4. random operands within the derived bound (K + 4) u (|scale| sum|w~ x~| + |shift|), u = 2^-23 - the f32 tests' bound
with one ulp per addition instead of half, so it holds whether the unit rounds to nearest or truncates - widened through SiLU and the
residual exactly as tests/test_gpu_yolox_net.py widens its own. 5. is part of every op (the tiles).
Whole nets: 6. the pooled RMS error against the f64 restatement is at most 2 x that of the bf16-operand emulations (one more draw of
the same rounding noise; the emulations differ from each other by at most 1.32 x). 7. bitwise properties, 8. the compositions,
9. the video group, 10. refusals and accounting."""
import numpy as np
import pytest

import test_gpu_group_yolox_infer as GI
import test_gpu_yolox_net as T
import yolox_net_bf16 as B
import yolox_net_cases as K
import yolox_net_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23          # one ulp per addition of the accumulator chain
U32 = T.U               # the f32 epilogue's unit, as the f32 tests widen with
SENTINEL = T.SENTINEL
CHANNELS = (1, 3, 4, 12, 24, 33, 65)
SPATIAL = ((1, 1), (2, 2), (5, 7), (9, 9))
Pool = T.Pool


def _run(ctx, kind, xw, x_view, wgt, scale, shift, k, stride, silu=False, resw=None, n=2):
    """The op under tiles 1, 4 and 0 on views; asserts the same bytes and the sentinel; returns the output view [n, cout, ho, wo]."""
    cout = wgt.shape[0]
    if kind == "focus":
        h, w = xw.shape[2] // 2, xw.shape[3] // 2
        in_c, in_off, in_ctot = 3, 0, 3
    else:
        h, w = xw.shape[2], xw.shape[3]
        in_c, in_off, in_ctot = x_view.shape[1], 1, xw.shape[1]
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    outw = np.full((n, cout + 3, ho, wo), SENTINEL, np.float32)
    with Pool(ctx) as D:
        args = dict(kind=kind, k=k, stride=stride, silu=int(silu), n_frames=n, h_in=h, w_in=w, inp=D.up(xw), in_c=in_c, in_off=in_off, in_ctot=in_ctot, out_c=cout,
                    out_off=2, out_ctot=cout + 3, res_off=1, res_ctot=cout + 1, res=None if resw is None else D.up(resw), weight=D.up(wgt),
                    scale=D.up(np.asarray(scale, np.float32)), shift=D.up(np.asarray(shift, np.float32)))
        got = []
        for tile in (1, 4, 0):
            d_out = D.up(outw)
            ctx.selftest_yolox_net_op_bf16(out=d_out, tile=tile, **args)
            got.append(D.down(d_out, outw))
    assert all((g.view(np.uint32) == got[0].view(np.uint32)).all() for g in got[1:]), "the tile shape changes no byte"
    assert (got[0][:, :2] == SENTINEL).all() and (got[0][:, 2 + cout:] == SENTINEL).all(), "the other channels of the wider buffer"
    return got[0][:, 2:2 + cout]


def _input(rng, n, c, h, w, ties=True):
    """[n, c + 2, h, w] normals with planted tie patterns (low half 0x8000 under an even and an odd upper half, 0x7FFF, 0x8001), no -0;
    the view's channels are 1 .. c"""
    xw = rng.normal(0.0, 1.0, (n, c + 2, h, w)).astype(np.float32)
    if ties:
        bits = xw.view(np.uint32).reshape(-1)
        lows = np.array([0x8000, 0x8000, 0x7FFF, 0x8001], np.uint32)
        pick = rng.integers(0, 8, bits.size)                       # half of the values get a pattern
        planted = pick < 4
        upper = bits & np.uint32(0xFFFF0000)
        upper = np.where(pick == 0, upper & np.uint32(0xFFFEFFFF), np.where(pick == 1, upper | np.uint32(0x00010000), upper))
        bits[planted] = (upper | lows[pick % 4])[planted]
    assert not ((xw == 0) & np.signbit(xw)).any() and np.isfinite(xw).all()
    return xw, xw[:, 1:1 + c]


def _same_values(got, want):
    want = np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.isfinite(got).all() and (got == want).all() and (got.view(np.uint32)[want != 0] == want.view(np.uint32)[want != 0]).all()


@pytest.mark.parametrize("h,w", SPATIAL)
def test_a_permutation_rounds_every_operand_to_nearest_even(ctx, h, w):
    """1: out channel o = bf16_round(in channel perm[o]), bit for bit: the rounding rule and the fragment maps (a cyclic shift is
    neither the identity nor symmetric from 3 channels on; 1 channel pins the rounding alone)."""
    rng = np.random.default_rng(400 + 10 * h + w)
    for c in CHANNELS:
        xw, x = _input(rng, 2, c, h, w)
        perm = (np.arange(c) + 1) % c
        wgt = np.zeros((c, c, 1, 1), np.float32)
        wgt[np.arange(c), perm] = 1.0
        assert c < 3 or not (wgt[:, :, 0, 0] == wgt[:, :, 0, 0].T).all()
        got = _run(ctx, "conv", xw, x, wgt, np.ones(c), np.zeros(c), 1, 1)
        want = B.bf16_round(x[:, perm])
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (c, h, w)
        assert (want != x[:, perm]).any()                                          # the operands do need rounding
        # a rectangular one: more output channels than inputs, each input read several times
        co = 65 if c != 65 else 33
        src = (np.arange(co) * 7 + 1) % c
        wgt = np.zeros((co, c, 1, 1), np.float32)
        wgt[np.arange(co), src] = 1.0
        got = _run(ctx, "conv", xw, x, wgt, np.ones(co), np.zeros(co), 1, 1)
        assert (got.view(np.uint32) == B.bf16_round(x[:, src]).view(np.uint32)).all(), (c, co, h, w)


@pytest.mark.parametrize("h,w", SPATIAL)
def test_one_tap_per_channel_pins_the_gather(ctx, h, w):
    """2: a 3 x 3 convolution with one tap of weight 1 per output channel, tap and source channel varying: the output is the shifted,
    zero-padded, rounded input, at stride 1 and 2 and through the Focus gather."""
    rng = np.random.default_rng(500 + 10 * h + w)
    for cin in CHANNELS:
        for cout in (4, 33, 65) if cin != 12 else CHANNELS:
            o = np.arange(cout)
            src, tap = (o * 5 + 2) % cin, (o * 4 + cin) % 9
            wgt = np.zeros((cout, cin, 3, 3), np.float32)
            wgt[o, src, tap // 3, tap % 3] = 1.0
            for stride in (1, 2):
                xw, x = _input(rng, 2, cin, h, w)
                got = _run(ctx, "conv", xw, x, wgt, np.ones(cout), np.zeros(cout), 3, stride)
                want = R.conv2d(B.bf16_round(x).astype(np.float64), wgt.astype(np.float64), stride, 1)
                assert _same_values(got, want), ("conv", cin, cout, h, w, stride)
            if cin == 12:
                frames = _input(rng, 2, 1, 2 * h, 2 * w)[0]                       # [2, 3, 2h, 2w]
                got = _run(ctx, "focus", frames, None, wgt, np.ones(cout), np.zeros(cout), 3, 1)
                want = R.conv2d(B.bf16_round(R.focus(frames)).astype(np.float64), wgt.astype(np.float64), 1, 1)
                assert _same_values(got, want), ("focus", cout, h, w)


@pytest.mark.parametrize("h,w", SPATIAL)
def test_small_integers_pin_the_whole_reduction(ctx, h, w):
    """3: inputs in [-8, 8], weights in [-4, 4], integer shifts: every partial sum is below 2^24 (65 x 9 x 32 < 2^15), so any order
    of summation is exact and the output is the integer convolution: the K tails, the tile tails and the accumulator chain."""
    rng = np.random.default_rng(600 + 10 * h + w)
    for cin, cout in ((65, 65), (33, 65), (65, 33), (24, 65), (4, 24), (65, 1)):
        for k in (1, 3):
            for stride in (1, 2):
                xw = rng.integers(-8, 9, (2, cin + 2, h, w)).astype(np.float32) + np.float32(0.0)
                wgt = rng.integers(-4, 5, (cout, cin, k, k)).astype(np.float32)
                shift = rng.integers(-3, 4, cout).astype(np.float32)
                got = _run(ctx, "conv", xw, xw[:, 1:1 + cin], wgt, np.ones(cout), shift, k, stride)
                want = R.conv2d(xw[:, 1:1 + cin].astype(np.float64), wgt.astype(np.float64), stride, (k - 1) // 2) + shift.reshape(1, -1, 1, 1)
                assert got.shape == want.shape and (got.astype(np.float64) == want).all(), (cin, cout, k, stride, h, w)
    frames = rng.integers(0, 256, (2, 3, 2 * h, 2 * w)).astype(np.float32)         # the stem: pixel values are exact
    wgt = rng.integers(-4, 5, (24, 12, 3, 3)).astype(np.float32)
    got = _run(ctx, "focus", frames, None, wgt, np.ones(24), np.zeros(24), 3, 1)
    assert (got.astype(np.float64) == R.conv2d(R.focus(frames).astype(np.float64), wgt.astype(np.float64), 1, 1)).all()


def test_small_integers_on_a_grid_where_the_forward_takes_the_wide_tile(ctx):
    """64 x 64 pixels, 65 channels, 2 frames: 64 x 2 x 2 = 256 wide blocks, at least three for every four of the MI355X's 256 compute
    units, so tile 0 - the forward's own rule - is the 64 x 64 form here; most blocks are interior ones, with no tail at all."""
    rng = np.random.default_rng(650)
    cin, cout, h, w = 33, 65, 64, 64
    for k, stride in ((3, 1), (1, 1)):
        xw = rng.integers(-8, 9, (2, cin + 2, h, w)).astype(np.float32)
        wgt = rng.integers(-4, 5, (cout, cin, k, k)).astype(np.float32)
        shift = rng.integers(-3, 4, cout).astype(np.float32)
        got = _run(ctx, "conv", xw, xw[:, 1:1 + cin], wgt, np.ones(cout), shift, k, stride)
        want = R.conv2d(xw[:, 1:1 + cin].astype(np.float64), wgt.astype(np.float64), stride, (k - 1) // 2) + shift.reshape(1, -1, 1, 1)
        assert got.shape == want.shape and (got.astype(np.float64) == want).all(), (k, stride)


def _random_op(ctx, rng, kind, cin, cout, h, w, k, stride, silu, res):
    """One op with random operands; the largest error / bound ratio (asserted <= 1)."""
    n = 2
    if kind == "focus":
        xw = rng.normal(0.0, 1.0, (n, 3, 2 * h, 2 * w)).astype(np.float32)
        x = R.focus(xw)
    else:
        xw, x = _input(rng, n, cin, h, w, ties=False)
    Kred = cin * k * k
    wgt = (rng.normal(0.0, 1.0, (cout, cin, k, k)) / np.sqrt(Kred)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = rng.normal(0.0, 0.5, cout).astype(np.float32)
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    resw = rng.normal(0.0, 1.0, (n, cout + 1, ho, wo)).astype(np.float32)
    got = _run(ctx, kind, xw, x, wgt, scale, shift, k, stride, silu, resw if res else None).astype(np.float64)
    x64, w64 = B.bf16_round(x).astype(np.float64), B.bf16_round(wgt).astype(np.float64)
    sc, sh = scale.astype(np.float64).reshape(1, -1, 1, 1), shift.astype(np.float64).reshape(1, -1, 1, 1)
    y = R.conv2d(x64, w64, stride, pad) * sc + sh
    bound = (Kred + 4) * U * (np.abs(sc) * R.conv2d(np.abs(x64), np.abs(w64), stride, pad) + np.abs(sh))
    if silu:
        y = R.silu(y)
        bound = 1.1 * bound + 8 * U32 * np.abs(y) + 2.0 ** -126
    if res:
        y = y + resw[:, 1:1 + cout].astype(np.float64)
        bound = bound * (1 + U32) + U32 * np.abs(y)
    assert got.shape == y.shape
    ratio = float((np.abs(got - y) / bound).max())
    assert ratio <= 1.0, (kind, cin, cout, h, w, k, stride, silu, res, ratio)
    return ratio


@pytest.mark.parametrize("h,w", SPATIAL)
def test_random_operands_within_the_derived_bound(ctx, h, w):
    """4: all four epilogues, each meeting every (k, stride)."""
    rng = np.random.default_rng(700 + 10 * h + w)
    worst, pair = 0.0, 0
    for cin in CHANNELS:
        for cout in CHANNELS:
            for j, (k, stride) in enumerate(((1, 1), (1, 2), (3, 1), (3, 2))):
                e = (pair + j) % 4
                worst = max(worst, _random_op(ctx, rng, "conv", cin, cout, h, w, k, stride, bool(e & 1), bool(e & 2)))
            pair += 1
    for cout in CHANNELS:
        for silu in (False, True):
            worst = max(worst, _random_op(ctx, rng, "focus", 12, cout, h, w, 3, 1, silu, False))
    print("bf16 dense conv %dx%d: largest error / bound %.3f" % (h, w, worst))


def test_every_epilogue_at_the_tile_tails(ctx):
    rng = np.random.default_rng(8)
    worst = 0.0
    for silu in (False, True):
        for res in (False, True):
            for k, stride in ((1, 1), (3, 1), (3, 2), (1, 2)):
                worst = max(worst, _random_op(ctx, rng, "conv", 65, 65, 9, 9, k, stride, silu, res))
                worst = max(worst, _random_op(ctx, rng, "conv", 33, 4, 9, 15, k, stride, silu, res))
    print("bf16 dense conv, every epilogue at the tails: largest error / bound %.3f" % worst)


# ---- whole nets

def _net(ctx, case, precision="bf16"):
    import mi355fx
    net = mi355fx.YoloxNet(ctx, case.cfg())
    try:
        assert net.precision() == 0                                                # the default
        net.set_precision(precision)
        net.load(case.P)
        net.finalize()
    except BaseException:
        net.close()
        raise
    assert net.precision() == (1 if precision == "bf16" else 0)
    return net


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.name)
def test_whole_net_pooled_rms_within_twice_the_emulations(ctx, case):
    """6: a case the guard of tests/yolox_net_bf16.py drops (at most 4, asserted on the CPU) is printed and not measured."""
    ratio = B.guard_ratio(case)
    if not B.GUARD[0] <= ratio <= B.GUARD[1]:
        print("%s: dropped by the guard, rms(emu32) / rms(emu64) = %.3f" % (case.name, ratio))
        assert len(B._guarded()[1]) <= B.MAX_DROPPED
        return
    ref64, emu64, emu32 = B.references(case)
    net = _net(ctx, case)
    try:
        with Pool(ctx) as D:
            got = T._forward(ctx, net, case.frames, D)
    finally:
        net.close()
    yard = max(B.pooled_rms(emu64, ref64), B.pooled_rms(emu32, ref64))
    err = B.pooled_rms(got, ref64)
    print("%s: pooled rms device %.4g, emu64 %.4g, emu32 %.4g, ratio %.3f" % (case.name, err, B.pooled_rms(emu64, ref64), B.pooled_rms(emu32, ref64), err / yard))
    for l in range(3):                                                             # informational: per map, against the larger emulation error
        for what, rows in K.MAPS:
            e = float(np.abs(got[l][:, rows] - ref64[l][:, rows]).max())
            y = max(float(np.abs(m[l][:, rows] - ref64[l][:, rows]).max()) for m in (emu64, emu32))
            print("  level %d %s: max-abs device %.4g, emulations %.4g, ratio %.3f" % (l, what, e, y, e / y if y else np.inf))
    assert all(np.isfinite(m).all() for m in got)
    assert err <= 2 * yard, (case.name, err, yard)


def test_the_same_call_twice_a_frame_alone_and_reversed(ctx):
    case = K.Case("tiny", 3, 64, 96, 3)
    net = _net(ctx, case)
    try:
        with Pool(ctx) as D:
            first = T._bits(T._forward(ctx, net, case.frames, D))
            assert T._same(first, T._bits(T._forward(ctx, net, case.frames, D)))
            for f in range(3):
                alone = T._bits(T._forward(ctx, net, case.frames[f:f + 1], D))
                assert T._same(alone, [m[f:f + 1] for m in first]), f
            swapped = T._bits(T._forward(ctx, net, case.frames[::-1], D))
            assert T._same(swapped, [m[::-1] for m in first])
    finally:
        net.close()


def test_a_batch_large_enough_for_the_wide_tile_is_its_frames_alone(ctx):
    """32 frames of s_width at 64 x 96: the stem (24 pixel tiles x 32 frames = 768 wide blocks) and dark2's layers (6 x 32 = 192) take
    the 64 x 64 tile under the forward's own rule, every forward of one frame the 64 x 16 tile throughout - the same bytes. The maps
    of a frame alone are the ones test 6 measures."""
    case = K.Case("s_width", 3, 64, 96, 3)
    batch = np.ascontiguousarray(case.frames[np.arange(32) % 3])
    net = _net(ctx, case)
    try:
        with Pool(ctx) as D:
            alone = [T._bits(T._forward(ctx, net, case.frames[f:f + 1], D)) for f in range(3)]
            got = T._bits(T._forward(ctx, net, batch, D))
        for i in range(32):
            assert T._same([m[i:i + 1] for m in got], alone[i % 3]), i
    finally:
        net.close()


def test_arena_regrowth_and_reuse(ctx):
    big, small = K.Case("nano", 3, 64, 96, 3), K.Case("nano", 3, 32, 32, 1)
    net = _net(ctx, big)
    try:
        with Pool(ctx) as D:
            b0 = T._bits(T._forward(ctx, net, big.frames, D))
            info = net.arena_info()
            s0 = T._bits(T._forward(ctx, net, small.frames, D))
            b1 = T._bits(T._forward(ctx, net, big.frames, D))
            assert T._same(b0, b1) and net.arena_info() == info
        fresh = _net(ctx, small)                                                   # ... and growing: 32 x 32 first
        try:
            with Pool(ctx) as D:
                assert T._same(s0, T._bits(T._forward(ctx, fresh, small.frames, D)))
                small_info = fresh.arena_info()
                assert T._same(b0, T._bits(T._forward(ctx, fresh, big.frames, D)))
                assert fresh.arena_info() == (info[0], small_info[1] + 1)
                assert T._same(s0, T._bits(T._forward(ctx, fresh, small.frames, D)))
        finally:
            fresh.close()
    finally:
        net.close()


def test_an_f32_net_and_a_bf16_net_side_by_side(ctx):
    case = K.Case("tiny", 3, 64, 96, 3)
    nf, nb = _net(ctx, case, "f32"), _net(ctx, case, "bf16")
    try:
        with Pool(ctx) as D:
            f0, b0 = T._bits(T._forward(ctx, nf, case.frames, D)), T._bits(T._forward(ctx, nb, case.frames, D))
            for _ in range(2):
                assert T._same(f0, T._bits(T._forward(ctx, nf, case.frames, D)))
                assert T._same(b0, T._bits(T._forward(ctx, nb, case.frames, D)))
            assert not any((x == y).all() for x, y in zip(f0, b0))                 # the mode is on
            # same config, same shape: the same op list and the same arena
            assert nf.launches() == nb.launches() and nf.arena_info() == nb.arena_info()
    finally:
        nf.close()
        nb.close()


@pytest.mark.parametrize("spec", [("nano", 3, 64, 96, 3), ("tiny", 1, 64, 96, 3)], ids=lambda s: "%s-c%d-%dx%d-n%d" % s)
def test_compositions_are_the_three_calls_by_hand(ctx, spec):
    case = K.CompositionCase(*spec)
    n, H, W, C, A = case.n, case.H, case.W, case.C, case.A
    net = _net(ctx, case)
    try:
        with Pool(ctx) as D:
            d_frames, pitch, stride = T._frames_on_device(case, D)
            F = 5 + C
            tensor = np.zeros((n, A, F), np.float32)
            d_t = D.up(tensor)
            net.infer_frames_device(d_frames, pitch, stride, n, W, H, d_t, A * F * 4)
            got_t = D.down(d_t, tensor)
            dets, counts = net.infer_dets_device(d_frames, pitch, stride, n, W, H, [case.params] * n, A, return_counts=True)
            x = np.zeros((n, 3, H, W), np.float32)
            d_x, d_t2 = D.up(x), D.up(tensor)
            ctx.yolox_input_frames_device(d_frames, pitch, stride, n, W, H, d_x, x[0].nbytes)
            levels = net.forward_device(d_x, x[0].nbytes, n, H, W)
            ctx.yolox_head_decode_device(levels, n, C, d_t2, A * F * 4)
            want_t = D.down(d_t2, tensor)
            want_dets, want_counts = ctx.yolox_head_dets_device(levels, n, C, [case.params] * n, A, return_counts=True)
        assert (got_t.view(np.uint32) == want_t.view(np.uint32)).all()
        assert list(counts) == list(want_counts) and sum(counts) >= 1
        for f in range(n):
            assert dets[f].tobytes() == want_dets[f].tobytes(), f
    finally:
        net.close()


def _member_equals_lone(member, result):
    got, n = result
    lone_got, lone_n = member.lone()
    assert n == lone_n and got.tobytes() == lone_got.tobytes(), member.name
    return n


def test_group_members_of_a_bf16_net(ctx):
    """9: three members share one BF16 net; a set that mixes a member of an F32 net and one of a BF16 net of the same parameters."""
    import mi355fx
    case = GI.case_of("nano", 3)
    nb, nf = _net(ctx, case, "bf16"), _net(ctx, case, "f32")
    members, g = [], mi355fx.Group(0)
    try:
        members = [GI.FrameMember(ctx, nb, case, f, *GI.LAYOUTS[f]) for f in range(3)]
        res = [g.wait_yolodec(t) for t in [m.submit(g) for m in members]]
        assert g.yolox_infer_stats()[:3] == (3, 1, 3)                              # one forward of three frames
        assert sum(_member_equals_lone(m, r) for m, r in zip(members, res)) >= 1
        mixed = [GI.FrameMember(ctx, nf, case, 0), GI.FrameMember(ctx, nb, case, 0)]
        members += mixed
        res = [g.wait_yolodec(t) for t in [m.submit(g) for m in mixed]]
        for m, r in zip(mixed, res):
            _member_equals_lone(m, r)
        # the two nets' maps of that frame differ, so each member did go through its own net
        with Pool(ctx) as D:
            a, b = T._forward(ctx, nf, case.frames[:1], D), T._forward(ctx, nb, case.frames[:1], D)
        assert not any((x == y).all() for x, y in zip(a, b))
    finally:
        GI._close(g, members, [nb, nf])


def test_refusals_leave_the_net_usable(ctx):
    import mi355fx
    INV = mi355fx.ERR_INVALID_ARG
    case = K.Case("nano", 1, 32, 32, 1)

    def status(fn, *a, **kw):
        with pytest.raises(mi355fx.Mi355Error) as e:
            fn(*a, **kw)
        return e.value.status

    assert ctx.L.mi355_yolox_net_set_precision(None, 1) == INV and ctx.L.mi355_yolox_net_precision(None) == INV
    net = mi355fx.YoloxNet(ctx, case.cfg())
    try:
        net.set_precision("bf16")
        net.load(case.P)
        for bad in (2, -1, 7):
            assert status(net.set_precision, bad) == INV
            assert net.precision() == 1
        net.set_precision("f32")                                                   # any number of times, after the parameters too:
        net.set_precision("bf16")                                                  # the last value holds
        net.finalize()
        assert status(net.set_precision, "f32") == INV and status(net.set_precision, "bf16") == INV and net.precision() == 1
        with Pool(ctx) as D:
            x = R.input_tensor(case.frames)
            d_x = D.up(x)
            def forwards():
                return T._bits(net.read_levels(net.forward_device(d_x, x[0].nbytes, 1, 32, 32), 1))

            def message(fn, *a, **kw):
                with pytest.raises(mi355fx.Mi355Error) as e:
                    fn(*a, **kw)
                assert e.value.status == INV
                return str(e.value)

            first = forwards()
            for prec in ("f32", "bf16", 5):                                        # after finalize, and unknown after finalize
                assert status(net.set_precision, prec) == INV
                assert T._same(first, forwards()) and net.precision() == 1
            assert ctx.L.mi355_yolox_net_set_precision(None, 1) == INV and T._same(first, forwards())
            buf = np.zeros((2, 4, 5, 7), np.float32)
            d_b, d_w = D.up(buf), D.up(np.ones((4, 4, 3, 3), np.float32))
            op = dict(k=3, stride=1, silu=0, n_frames=2, h_in=5, w_in=7, inp=d_b, in_c=4, in_off=0, in_ctot=4, out_c=4, out=d_b, out_off=0, out_ctot=4, weight=d_w,
                      scale=d_w, shift=d_w)
            for kind in ("dw", "pool5", "up2"):                                    # kinds 1 to 3: valid ops of the f32 entry, refused for their kind
                ctx.selftest_yolox_net_op(kind=kind, **dict(op, out=D.up(np.zeros((2, 4, 10, 14), np.float32))))
                assert "neither a dense conv nor the Focus stem" in message(ctx.selftest_yolox_net_op_bf16, kind=kind, **op), kind
                assert T._same(first, forwards()), kind
            assert "tile" in message(ctx.selftest_yolox_net_op_bf16, kind="conv", tile=2, **op)          # a tile that names no shape
            assert T._same(first, forwards())
            ctx.selftest_yolox_net_op_bf16(kind="conv", tile=0, **dict(op, out=D.up(buf)))               # the same op with a tile that exists
            again = forwards()
            assert T._same(first, again)
            plain = _net(ctx, case, "f32")
            try:
                plain.read_levels(plain.forward_device(d_x, x[0].nbytes, 1, 32, 32), 1)
                assert plain.launches() == net.launches() and plain.arena_info() == net.arena_info()
            finally:
                plain.close()
        ref64, emu64, emu32 = B.references(case)
        got = [m.view(np.float32) for m in first]
        assert B.pooled_rms(got, ref64) <= 2 * max(B.pooled_rms(emu64, ref64), B.pooled_rms(emu32, ref64))
    finally:
        net.close()
