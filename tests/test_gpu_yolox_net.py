"""yoloxinference's network on the GPU (csrc/yolox_net.hip) against the numpy restatement (tests/yolox_net_restate.py;
cases: tests/yolox_net_cases.py).

1. Single ops through the test-only entry mi355_selftest_yolox_net_op_device (a plan of one op on caller views - chosen over a debug
   tap because it reaches channel counts and sizes no stock net has), with a DERIVED bound: u = 2^-24, K = Cin / groups * k^2,
   |err_pre| <= (K + 4) u (|scale| sum|w x| + |shift|) - the standard bound of a K-term sum in any order plus the epilogue's roundings -
   and after SiLU 1.1 err_pre + 8 u |silu(y)| + 2^-126. A residual is one more f32 add: e (1 + u) + u |out|. Pool and upsample are
   bit-exact. Every op writes at a nonzero channel offset into a wider buffer whose other channels hold a sentinel that must survive.
   A dense convolution runs under both tile shapes of its kernel and under the forward's own choice: the same bytes.
2. Whole nets: the device's raw maps against the f64 restatement; the yardstick is the f32 restatement's own max-abs error against
   f64 per map (measured here on the CPU), the device may have 4 x that. Both figures are printed per map.
3. Bitwise properties. 4. The two compositions, bit for bit. 5. Launch and allocation accounting; the refusals that need a device."""
import numpy as np
import pytest

import yolox_net_cases as K
import yolox_net_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = np.float32(7e30)
CHANNELS = (1, 3, 4, 12, 24, 65)
SPATIAL = ((1, 1), (2, 2), (5, 7))


class Pool:
    """device allocations of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.ctx.alloc(max(arr.nbytes, 16))
        self.ptrs.append(d)
        self.ctx.h2d(d, arr)
        return d

    def down(self, d, like):
        out = np.empty_like(like)
        self.ctx.synchronize()
        self.ctx.d2h(out, d)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for d in self.ptrs:
            self.ctx.free(d)


def _wide(rng, n, c, off, extra, h, w, fill=None):
    """[n, c + extra, h, w] f32: the view's channels are off .. off + c"""
    a = rng.normal(0.0, 1.0, (n, c + extra, h, w)).astype(np.float32) if fill is None else np.full((n, c + extra, h, w), fill, np.float32)
    return a, a[:, off:off + c]


def _conv_op(ctx, rng, kind, cin, cout, h, w, k, stride, silu, res, n=2):
    """One convolution op on views; returns the largest error / bound ratio (asserted <= 1)."""
    groups = cin if kind == "dw" else 1
    if kind == "focus":
        xw = rng.normal(0.0, 1.0, (n, 3, 2 * h, 2 * w)).astype(np.float32)
        x, in_off, in_ctot, in_c = R.focus(xw), 0, 3, 3
    else:
        xw, x = _wide(rng, n, cin, 1, 2, h, w)
        in_off, in_ctot, in_c = 1, cin + 2, cin
    Kred = (cin // groups) * k * k
    wgt = (rng.normal(0.0, 1.0, (cout, cin // groups, k, k)) / np.sqrt(Kred)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = rng.normal(0.0, 0.5, cout).astype(np.float32)
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    outw, _ = _wide(rng, n, cout, 2, 3, ho, wo, SENTINEL)
    resw, r = _wide(rng, n, cout, 1, 1, ho, wo)
    with Pool(ctx) as D:
        args = dict(kind=kind, k=k, stride=stride, silu=int(silu), n_frames=n, h_in=h, w_in=w, inp=D.up(xw), in_c=in_c, in_off=in_off, in_ctot=in_ctot, out_c=cout,
                    out_off=2, out_ctot=cout + 3, res_off=1, res_ctot=cout + 1, res=D.up(resw) if res else None, weight=D.up(wgt), scale=D.up(scale),
                    shift=D.up(shift))
        got_by_tile = []
        for tile in ((0,) if kind == "dw" else (1, 4, 0)):           # the dense kernel's two tile shapes, and the forward's own choice
            d_out = D.up(outw)
            ctx.selftest_yolox_net_op(out=d_out, tile=tile, **args)
            got_by_tile.append(D.down(d_out, outw))
        got_w = got_by_tile[0]
        assert all((g.view(np.uint32) == got_w.view(np.uint32)).all() for g in got_by_tile[1:]), "the tile shape changes no byte"
    assert (got_w[:, :2] == SENTINEL).all() and (got_w[:, 2 + cout:] == SENTINEL).all(), "the other channels of the wider buffer"
    got = got_w[:, 2:2 + cout].astype(np.float64)
    x64, w64 = x.astype(np.float64), wgt.astype(np.float64)
    sc, sh = scale.astype(np.float64).reshape(1, -1, 1, 1), shift.astype(np.float64).reshape(1, -1, 1, 1)
    y = R.conv2d(x64, w64, stride, pad, groups) * sc + sh
    bound = (Kred + 4) * U * (np.abs(sc) * R.conv2d(np.abs(x64), np.abs(w64), stride, pad, groups) + np.abs(sh))
    if silu:
        y = R.silu(y)
        bound = 1.1 * bound + 8 * U * np.abs(y) + 2.0 ** -126
    if res:
        y = y + r.astype(np.float64)
        bound = bound * (1 + U) + U * np.abs(y)
    assert got.shape == y.shape
    ratio = float((np.abs(got - y) / bound).max())
    assert ratio <= 1.0, (kind, cin, cout, h, w, k, stride, silu, res, ratio)
    return ratio


@pytest.mark.parametrize("h,w", SPATIAL)
def test_dense_conv_ops_within_the_derived_bound(ctx, h, w):
    rng = np.random.default_rng(100 + h * 10 + w)
    worst, pair = 0.0, 0
    for cin in CHANNELS:
        for cout in CHANNELS:
            for j, (k, stride) in enumerate(((1, 1), (1, 2), (3, 1), (3, 2))):
                e = (pair + j) % 4                                # the four epilogues in turn: every (k, stride) meets each of them
                worst = max(worst, _conv_op(ctx, rng, "conv", cin, cout, h, w, k, stride, bool(e & 1), bool(e & 2)))
            pair += 1
    print("dense conv %dx%d: largest error / bound %.3f" % (h, w, worst))


def test_dense_conv_every_epilogue_at_the_tile_tails(ctx):
    rng = np.random.default_rng(7)
    for silu in (False, True):
        for res in (False, True):
            for k, stride in ((1, 1), (3, 1), (3, 2), (1, 2)):
                _conv_op(ctx, rng, "conv", 65, 65, 5, 7, k, stride, silu, res)          # two channel tiles, a 16-step tail in the reduction
                _conv_op(ctx, rng, "conv", 24, 4, 9, 15, k, stride, silu, res, n=3)     # more than one pixel tile at stride 1


@pytest.mark.parametrize("h,w", SPATIAL)
def test_depthwise_ops_within_the_derived_bound(ctx, h, w):
    rng = np.random.default_rng(200 + h * 10 + w)
    worst = 0.0
    for i, c in enumerate(CHANNELS):
        for stride in (1, 2):
            for silu in (False, True):
                worst = max(worst, _conv_op(ctx, rng, "dw", c, c, h, w, 3, stride, silu, bool((i + stride) & 1)))
    _conv_op(ctx, rng, "dw", 3, 3, 17, 19, 3, 1, True, True)                             # more than one block of 256 pixels
    print("depthwise %dx%d: largest error / bound %.3f" % (h, w, worst))


@pytest.mark.parametrize("h,w", SPATIAL)
def test_focus_stem_ops_within_the_derived_bound(ctx, h, w):
    rng = np.random.default_rng(300 + h * 10 + w)
    for cout in CHANNELS:
        for silu in (False, True):
            _conv_op(ctx, rng, "focus", 12, cout, h, w, 3, 1, silu, False)


@pytest.mark.parametrize("kind", ["pool5", "up2"])
def test_pool_and_upsample_are_bit_exact(ctx, kind):
    rng = np.random.default_rng(5)
    for c in CHANNELS:
        for h, w in SPATIAL + ((13, 21),):
            n = 2
            xw, x = _wide(rng, n, c, 1, 2, h, w)
            xw -= np.float32(4.0)                                                        # all negative: a zero pad would win
            want = R.max_pool(x, 5) if kind == "pool5" else R.upsample2(x)
            outw, _ = _wide(rng, n, c, 2, 3, want.shape[2], want.shape[3], SENTINEL)
            with Pool(ctx) as D:
                d_out = D.up(outw)
                ctx.selftest_yolox_net_op(kind=kind, k=0, stride=1, silu=0, n_frames=n, h_in=h, w_in=w, inp=D.up(xw), in_c=c, in_off=1, in_ctot=c + 2, out_c=c,
                                          out=d_out, out_off=2, out_ctot=c + 3)
                got = D.down(d_out, outw)
            assert (got[:, :2] == SENTINEL).all() and (got[:, 2 + c:] == SENTINEL).all()
            assert (got[:, 2:2 + c].view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all(), (kind, c, h, w)


def test_spp_cascade_in_place_in_one_buffer(ctx):
    """SPP's placement: pool 5 three times inside ONE concat buffer, channel group i + 1 from group i."""
    rng = np.random.default_rng(6)
    hid, h, w, n = 3, 5, 7, 2
    buf = rng.normal(-2.0, 1.0, (n, 4 * hid, h, w)).astype(np.float32)
    with Pool(ctx) as D:
        d = D.up(buf)
        for i in range(1, 4):
            ctx.selftest_yolox_net_op(kind="pool5", k=0, stride=1, silu=0, n_frames=n, h_in=h, w_in=w, inp=d, in_c=hid, in_off=(i - 1) * hid, in_ctot=4 * hid,
                                      out_c=hid, out=d, out_off=i * hid, out_ctot=4 * hid)
        got = D.down(d, buf)
    x = buf[:, :hid]
    assert (got == np.concatenate([x] + [R.max_pool(x, k) for k in R.SPP_POOLING], axis=1)).all()


# ---- whole nets

def _device_net(ctx, case):
    import mi355fx
    net = mi355fx.YoloxNet(ctx, case.cfg())
    net.load(case.P)
    net.finalize()
    return net


def _forward(ctx, net, frames_u8, D):
    x = R.input_tensor(frames_u8)
    n, _, H, W = x.shape
    levels = net.forward_device(D.up(x), x[0].nbytes, n, H, W)
    return net.read_levels(levels, n)


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.name)
def test_whole_net_within_four_times_the_f32_restatement(ctx, case):
    ref64, ref32 = case.ref(np.float64), case.ref(np.float32)
    net = _device_net(ctx, case)
    try:
        with Pool(ctx) as D:
            got = _forward(ctx, net, case.frames, D)
    finally:
        net.close()
    failures = []
    for l in range(3):
        assert got[l].shape == ref64[l].shape
        for what, rows in (("reg", slice(0, 4)), ("obj", slice(4, 5)), ("cls", slice(5, None))):
            yard = float(np.abs(ref32[l][:, rows].astype(np.float64) - ref64[l][:, rows]).max())
            err = float(np.abs(got[l][:, rows].astype(np.float64) - ref64[l][:, rows]).max())
            print("%s level %d %s: device %.4g, f32 restatement %.4g, ratio %.3f (map max %.4g)" % (case.name, l, what, err, yard, err / yard if yard else np.inf,
                                                                                                    np.abs(ref64[l][:, rows]).max()))
            if not err <= 4 * yard:
                failures.append((l, what, err, yard))
    assert not failures, failures


# ---- bitwise properties

def _bits(maps):
    return [m.view(np.uint32).copy() for m in maps]


def _same(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def test_the_same_call_twice_and_a_frame_alone(ctx):
    case = K.Case("tiny", 3, 64, 96, 3)
    net = _device_net(ctx, case)
    try:
        with Pool(ctx) as D:
            first = _bits(_forward(ctx, net, case.frames, D))
            assert _same(first, _bits(_forward(ctx, net, case.frames, D)))
            for f in range(3):                                        # frame f of the batch of three equals that frame alone
                alone = _bits(_forward(ctx, net, case.frames[f:f + 1], D))
                assert _same(alone, [m[f:f + 1] for m in first]), f
            swapped = _bits(_forward(ctx, net, case.frames[::-1], D))    # ... and does not depend on its position
            assert _same(swapped, [m[::-1] for m in first])
    finally:
        net.close()


def test_arena_regrowth_and_reuse(ctx):
    big, small = K.Case("nano", 3, 64, 96, 3), K.Case("nano", 3, 32, 32, 1)
    net = _device_net(ctx, small)
    try:
        with Pool(ctx) as D:
            s0 = _bits(_forward(ctx, net, small.frames, D))
            bytes_small, allocs_small = net.arena_info()
            b0 = _bits(_forward(ctx, net, big.frames, D))              # the arena grows
            bytes_big, allocs_big = net.arena_info()
            assert bytes_big > bytes_small and allocs_big == allocs_small + 1
            s1 = _bits(_forward(ctx, net, small.frames, D))            # planned again inside the larger arena
            b1 = _bits(_forward(ctx, net, big.frames, D))
            assert _same(s0, s1) and _same(b0, b1)
            assert net.arena_info() == (bytes_big, allocs_big)         # a seen shape allocates nothing
        import mi355fx
        rc, plan = mi355fx.selftest_yolox_net_plan(big.cfg(), 3, 64, 96)
        assert rc == 0 and plan.arena_bytes == bytes_big
    finally:
        net.close()


def test_two_nets_on_one_context(ctx):
    a, b = K.Case("tiny", 3, 64, 96, 3), K.Case("nano", 1, 32, 32, 1)
    na, nb = _device_net(ctx, a), _device_net(ctx, b)
    try:
        with Pool(ctx) as D:
            xa, xb = R.input_tensor(a.frames), R.input_tensor(b.frames)
            la = na.forward_device(D.up(xa), xa[0].nbytes, 3, 64, 96)
            lb = nb.forward_device(D.up(xb), xb[0].nbytes, 1, 32, 32)    # the other net's forward must leave la's maps alone
            got_a, got_b = _bits(na.read_levels(la, 3)), _bits(nb.read_levels(lb, 1))
            assert _same(got_a, _bits(_forward(ctx, na, a.frames, D))) and _same(got_b, _bits(_forward(ctx, nb, b.frames, D)))
    finally:
        na.close()
        nb.close()


# ---- the compositions

COMPOSITIONS = [(c, 3, 64, 96, 3) for c in K.CONFIGS] + [("nano", 1, 32, 32, 1), ("tiny", 3, 32, 32, 3)]


def _frames_on_device(case, D, pad=5):
    """packed RGB rows with `pad` bytes of row padding and a frame pitch with a gap"""
    n, H, W, _ = case.frames.shape
    stride = 3 * W + pad
    pitch = H * stride + 11
    buf = np.full(n * pitch, 201, np.uint8)
    for f in range(n):
        rows = buf[f * pitch:f * pitch + H * stride].reshape(H, stride)
        rows[:, :3 * W] = case.frames[f].reshape(H, 3 * W)
    return D.up(buf), pitch, stride


@pytest.mark.parametrize("spec", COMPOSITIONS, ids=lambda s: "%s-c%d-%dx%d-n%d" % s)
def test_compositions_bit_for_bit(ctx, spec):
    case = K.CompositionCase(*spec)
    n, H, W, C, A = case.n, case.H, case.W, case.C, case.A
    net = _device_net(ctx, case)
    try:
        with Pool(ctx) as D:
            d_frames, pitch, stride = _frames_on_device(case, D)
            F = 5 + C
            tensor = np.zeros((n, A, F), np.float32)
            d_t = D.up(tensor)
            net.infer_frames_device(d_frames, pitch, stride, n, W, H, d_t, A * F * 4)
            got_t = D.down(d_t, tensor)
            dets, counts = net.infer_dets_device(d_frames, pitch, stride, n, W, H, [case.params] * n, A, return_counts=True)
            # the chain by hand, on the same stream
            x = np.zeros((n, 3, H, W), np.float32)
            d_x, d_t2 = D.up(x), D.up(tensor)
            ctx.yolox_input_frames_device(d_frames, pitch, stride, n, W, H, d_x, x[0].nbytes)
            levels = net.forward_device(d_x, x[0].nbytes, n, H, W)
            ctx.yolox_head_decode_device(levels, n, C, d_t2, A * F * 4)
            want_t = D.down(d_t2, tensor)
            want_dets, want_counts = ctx.yolox_head_dets_device(levels, n, C, [case.params] * n, A, return_counts=True)
            assert (D.down(d_x, x) == R.input_tensor(case.frames)).all()
        assert (got_t.view(np.uint32) == want_t.view(np.uint32)).all()
        assert list(counts) == list(want_counts)
        for f in range(n):
            assert dets[f].tobytes() == want_dets[f].tobytes(), f
            assert 1 <= counts[f] <= case.survivors[f] <= A // 2, (counts[f], case.survivors[f])   # NMS keeps some of the survivors
        # the decoded tensor is the network's: its objectness column against the f64 maps, well inside the thresholds' guard
        obj64 = np.concatenate([K.sigmoid64(m[:, 4]).reshape(n, -1) for m in case.maps64], axis=1)
        assert np.abs(got_t[:, :, 4] - obj64).max() < 2e-5
    finally:
        net.close()


# ---- accounting and refusals

def test_launch_and_allocation_accounting(ctx):
    import mi355fx
    for config in ("nano", "tiny", "deep_c3"):
        case = K.CompositionCase(config, 3, 64, 96, 3)
        rc, plan = mi355fx.selftest_yolox_net_plan(case.cfg(), 3, 64, 96)
        net = _device_net(ctx, case)
        try:
            assert rc == 0 and net.launches() == plan.launches and net.param_count() == plan.param_count
            assert net.params() == mi355fx.selftest_yolox_net_params(case.cfg())
            with Pool(ctx) as D:
                d_frames, pitch, stride = _frames_on_device(case, D)
                first = net.infer_dets_device(d_frames, pitch, stride, 3, 96, 64, [case.params] * 3, case.A)
                info = net.arena_info()
                assert info[1] == 2                                      # the arena and the compositions' input tensor
                h2d = ctx.transfer_counts()[0]
                again = net.infer_dets_device(d_frames, pitch, stride, 3, 96, 64, [case.params] * 3, case.A)
                assert net.arena_info() == info                          # a second call at a seen shape allocates nothing
                assert ctx.transfer_counts()[0] - h2d <= 1               # and uploads nothing but the decoder's settings
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        finally:
            net.close()


def test_refusals_leave_the_net_usable(ctx):
    import mi355fx
    INV, UNS, NOT = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED, mi355fx.ERR_NOT_CONFIGURED
    case = K.Case("nano", 1, 32, 32, 1)

    def status(fn, *a, **kw):
        with pytest.raises(mi355fx.Mi355Error) as e:
            fn(*a, **kw)
        return e.value.status

    assert status(mi355fx.YoloxNet, ctx, mi355fx.yolox_net_config(0.5, 0.25, True, 1)) == INV
    assert status(mi355fx.YoloxNet, ctx, mi355fx.yolox_net_config(0.33, 0.25, True, 1, 7)) == INV
    assert status(mi355fx.YoloxNet, ctx, mi355fx.yolox_net_config(0.33, 0.25, True, 2000)) == UNS
    net = mi355fx.YoloxNet(ctx, case.cfg())
    try:
        table = net.params()
        with Pool(ctx) as D:
            x = R.input_tensor(case.frames)
            d_x = D.up(x)
            assert status(net.forward_device, d_x, x[0].nbytes, 1, 32, 32) == NOT
            for k, (name, dims) in enumerate(table[:-1]):
                net.set_param(k, case.P[name])
            assert status(net.finalize) == INV                              # one parameter is still unset
            last = case.P[table[-1][0]]
            assert status(net.set_param, len(table) - 1, np.zeros(last.size + 1, np.float32)) == INV      # a wrong element count
            assert status(net.set_param, len(table), last) == INV
            assert status(net.finalize) == INV
            net.set_param(len(table) - 1, last)
            net.finalize()
            assert status(net.set_param, 0, case.P[table[0][0]]) == INV      # immutable from now on
            for args, want in (((0, 32, 32), INV), ((65, 32, 32), UNS), ((1, 33, 32), INV), ((1, 32, 16), INV), ((1, 2080, 32), UNS)):
                assert status(net.forward_device, d_x, x[0].nbytes, *args) == want, args
            assert status(net.forward_device, None, x[0].nbytes, 1, 32, 32) == INV
            assert status(net.forward_device, d_x, 8, 3, 32, 32) == INV      # a pitch below the tensor
            got = net.read_levels(net.forward_device(d_x, x[0].nbytes, 1, 32, 32), 1)
        ref64 = case.ref(np.float64)
        for l in range(3):
            assert np.abs(got[l] - ref64[l]).max() <= 1e-4 * np.abs(ref64[l]).max()
    finally:
        net.close()
