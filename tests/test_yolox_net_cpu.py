"""CPU tests of yoloxinference's network (csrc/yolox_net.hip): the restatement's known answers by hand, the library's
host-only plan and parameter enumeration against the restatement for the six stock variants, every refusal that needs no device, and -
where torch imports - the restatement against torch.nn.functional on the CPU, which pins padding, pooling and concat order a third
time."""
import numpy as np
import pytest

import yolox_net_cases as K
import yolox_net_restate as R


# ---- known answers of the restatement

def test_focus_channel_order_on_a_2x2_frame():
    x = np.arange(12, dtype=np.float64).reshape(1, 3, 2, 2)          # channel c: [[4c, 4c + 1], [4c + 2, 4c + 3]]
    got = R.focus(x).reshape(12)
    # top-left of r, g, b; bottom-left; top-right; bottom-right (blocks.rs:200-208)
    assert got.tolist() == [0, 4, 8, 2, 6, 10, 1, 5, 9, 3, 7, 11]


def test_max_pool_padding_never_wins():
    one = np.full((1, 1, 1, 1), -3.0)
    for k in R.SPP_POOLING:
        assert R.max_pool(one, k).tolist() == [[[[-3.0]]]]             # a zero pad would give 0
    two = np.array([[[[-1.0, -2.0], [-3.0, -4.0]]]])
    assert (R.max_pool(two, 5) == -1.0).all()
    x = np.random.default_rng(1).normal(size=(2, 3, 7, 9)) - 5.0
    assert (R.max_pool(R.max_pool(x, 5), 5) == R.max_pool(x, 9)).all()                      # 9 = 5 o 5, exactly
    assert (R.max_pool(R.max_pool(R.max_pool(x, 5), 5), 5) == R.max_pool(x, 13)).all()      # 13 = 5 o 5 o 5


def _conv_by_hand(x, w, stride):
    h, wd = x.shape
    ho, wo = (h + 2 - 3) // stride + 1, (wd + 2 - 3) // stride + 1
    out = np.zeros((ho, wo))
    for oy in range(ho):
        for ox in range(wo):
            for dy in range(3):
                for dx in range(3):
                    iy, ix = oy * stride - 1 + dy, ox * stride - 1 + dx
                    if 0 <= iy < h and 0 <= ix < wd:
                        out[oy, ox] += w[dy, dx] * x[iy, ix]
    return out


def test_conv_3x3_stride_2_pad_1_by_hand():
    w = np.arange(1.0, 10.0).reshape(3, 3)
    x2 = np.array([[1.0, 2.0], [3.0, 4.0]])
    got = R.conv2d(x2.reshape(1, 1, 2, 2), w.reshape(1, 1, 3, 3), 2, 1)
    assert got.shape == (1, 1, 1, 1)
    assert got[0, 0, 0, 0] == 5 * 1 + 6 * 2 + 8 * 3 + 9 * 4          # three of the four tap rows / columns are padding
    x4 = np.arange(16.0).reshape(4, 4) - 7.0
    got = R.conv2d(x4.reshape(1, 1, 4, 4), w.reshape(1, 1, 3, 3), 2, 1)
    assert got.shape == (1, 1, 2, 2) and (got[0, 0] == _conv_by_hand(x4, w, 2)).all()
    assert got[0, 0, 0, 0] == 5 * -7 + 6 * -6 + 8 * -3 + 9 * -2
    got1 = R.conv2d(x4.reshape(1, 1, 4, 4), w.reshape(1, 1, 3, 3), 1, 1)
    assert (got1[0, 0] == _conv_by_hand(x4, w, 1)).all()


def test_depthwise_and_multi_channel_conv():
    rng = np.random.default_rng(2)
    x, w = rng.normal(size=(2, 3, 5, 7)), rng.normal(size=(3, 1, 3, 3))
    got = R.conv2d(x, w, 2, 1, groups=3)
    for n in range(2):
        for c in range(3):
            assert np.allclose(got[n, c], _conv_by_hand(x[n, c], w[c, 0], 2), rtol=0, atol=1e-13)
    w = rng.normal(size=(4, 3, 3, 3))
    got = R.conv2d(x, w, 1, 1)
    want = sum(_conv_by_hand(x[1, c], w[2, c], 1) for c in range(3))
    assert np.allclose(got[1, 2], want, rtol=0, atol=1e-13)


def test_nearest_upsample():
    x = np.array([[[[1.0, 2.0], [3.0, 4.0]]]])
    assert R.upsample2(x)[0, 0].tolist() == [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]]


def test_residual_is_added_after_silu():
    b = R.Bottleneck("b", 1, 1, True, False)
    P = {"b.conv1.conv.weight": np.ones((1, 1, 1, 1)), "b.conv2.conv.weight": np.zeros((1, 1, 3, 3))}
    P["b.conv2.conv.weight"][0, 0, 1, 1] = 1.0
    for c in ("b.conv1", "b.conv2"):
        P[c + ".bn.weight"], P[c + ".bn.bias"], P[c + ".bn.running_mean"] = np.ones(1), np.zeros(1), np.zeros(1)
        P[c + ".bn.running_var"] = np.full(1, 1.0 - R.BN_EPS)
    x = np.full((1, 1, 1, 1), -2.0)
    s = lambda v: v / (1.0 + np.exp(-v))
    want = s(s(-2.0)) + -2.0                    # silu(x + identity) would be another number
    assert abs(b.fwd(P, x, None)[0, 0, 0, 0] - want) < 1e-15 and abs(want - s(s(-2.0) - 2.0)) > 0.1


def test_expand_and_block_counts():
    assert R.expand(64, 0.375) == 24 and R.expand(256, 0.375) == 96 and R.expand(64, 1.25) == 80 and R.expand(1024, 0.25) == 256
    assert [R.base_depth(d) for d in R.DEPTHS] == [1, 2, 3, 4]
    assert [R.num_blocks(d) for d in R.DEPTHS] == [1, 2, 3, 4]
    net = R.Yolox(0.67, 0.25, False, 1)
    assert len(net.backbone.backbone.dark2.c3.m) == 2 and len(net.backbone.backbone.dark3.c3.m) == 6 and len(net.backbone.c3_p4.m) == 2
    assert net.backbone.backbone.dark3.c3.m[0].shortcut and not net.backbone.backbone.dark5.c3.m[0].shortcut and not net.backbone.c3_n3.m[0].shortcut


def test_state_dict_names():
    names = {n for n, _ in R.Yolox(0.33, 0.375, False, 80).params}
    for must in ("backbone.backbone.dark3.c3.m.0.conv2.conv.weight", "head.cls_convs.1.conv0.conv.weight", "backbone.backbone.stem.conv.bn.running_var",
                 "backbone.backbone.dark5.spp.conv2.conv.weight", "backbone.c3_p4.m.0.conv1.bn.bias", "head.obj_preds.2.bias", "head.reg_preds.0.weight"):
        assert must in names, must
    names = {n for n, _ in R.Yolox(0.33, 0.25, True, 80).params}
    for must in ("backbone.backbone.dark2.conv.dconv.conv.weight", "backbone.bu_conv1.pconv.bn.weight", "head.reg_convs.2.conv1.dconv.conv.weight"):
        assert must in names, must


# ---- the library's host-only plan and enumeration

@pytest.mark.parametrize("variant", list(K.STOCK))
def test_plan_and_enumeration_match_the_restatement(mi355lib, variant):
    import mi355fx
    depth, width, dw = K.STOCK[variant]
    assert mi355fx.YOLOX_VARIANTS[variant] == (depth, width, dw)
    net = R.Yolox(depth, width, dw, 80)
    cfg = mi355fx.yolox_net_config(depth, width, dw, 80)
    H, W = 64, 96
    rc, plan = mi355fx.selftest_yolox_net_plan(cfg, 2, H, W)
    assert rc == 0 and (plan.status, plan.config_status, plan.frames_status, plan.size_status) == (0, 0, 0, 0)
    table = mi355fx.selftest_yolox_net_params(cfg)
    assert table == [(n, tuple(s)) for n, s in net.params]              # names, order and dims
    assert plan.param_count == len(net.params) and plan.param_floats == net.param_floats()
    assert [(plan.level_h[l], plan.level_w[l]) for l in range(3)] == [(H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
    assert plan.launches > 0 and plan.arena_bytes > 0 and plan.macs > 0
    rc, plan1 = mi355fx.selftest_yolox_net_plan(cfg, 1, H, W)
    assert plan1.macs * 2 == plan.macs and plan1.launches == plan.launches
    # one index past the table is refused
    import ctypes as C
    L = mi355lib
    name, dims, nd = C.create_string_buffer(96), (C.c_uint32 * 4)(), C.c_int(0)
    assert L.mi355_selftest_yolox_net_param_info(C.byref(cfg), len(net.params), name, 96, dims, C.byref(nd)) == mi355fx.ERR_INVALID_ARG
    assert L.mi355_selftest_yolox_net_param_info(C.byref(cfg), 0, name, 8, dims, C.byref(nd)) == mi355fx.ERR_INVALID_ARG      # a name buffer too small


def test_macs_of_yolox_s_are_the_published_count(mi355lib):
    import mi355fx
    rc, plan = mi355fx.selftest_yolox_net_plan(mi355fx.yolox_net_config(0.33, 0.5, False, 80), 1, 640, 640)
    assert rc == 0 and abs(2 * plan.macs / 1e9 - 26.8) < 0.3            # YOLOX-s: 26.8 GFLOPs at 640 x 640 (arXiv 2107.08430, table 6)


def test_refusals_that_need_no_device(mi355lib):
    import mi355fx
    INV, UNS = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED
    cfg = lambda *a: mi355fx.yolox_net_config(*a)
    plan = lambda c, n=1, H=32, W=32: mi355fx.selftest_yolox_net_plan(c, n, H, W)
    for depth in R.DEPTHS:
        for width in R.WIDTHS:
            assert plan(cfg(depth, width, False, 2))[0] == 0, (depth, width)
    for bad, status in ((cfg(0.5, 0.5, False, 1), INV), (cfg(0.33, 0.3, False, 1), INV), (cfg(0.330001, 0.5, False, 1), INV), (cfg(0.33, 0.5, 2, 1), INV),
                        (cfg(0.33, 0.5, -1, 1), INV), (cfg(0.33, 0.5, False, 0), INV), (cfg(0.33, 0.5, False, 1, 1), INV), (cfg(0.33, 0.5, False, 1025), UNS),
                        (None, INV)):
        rc, p = plan(bad)
        assert rc == status and p.status == status and p.config_status == status and p.frames_status == 0 and p.size_status == 0
    assert plan(cfg(0.33, 0.5, False, 1024))[0] == 0
    good = cfg(0.33, 0.25, True, 1)
    for n, status in ((0, INV), (-1, INV), (65, UNS), (64, 0)):
        rc, p = plan(good, n)
        assert rc == status and p.frames_status == status and p.config_status == 0 and p.size_status == 0, n
    for (H, W), status in (((0, 32), INV), ((32, 0), INV), ((33, 32), INV), ((32, 48), INV), ((2049, 32), INV), ((2080, 32), UNS), ((32, 2080), UNS),
                           ((2048, 2048), 0)):
        rc, p = plan(good, 1, H, W)
        assert rc == status and p.size_status == status and p.config_status == 0 and p.frames_status == 0, (H, W)
    rc, p = plan(cfg(0.5, 0.5, False, 1), 65, 33, 32)                  # the first refusal wins, every status is reported
    assert rc == INV and (p.config_status, p.frames_status, p.size_status) == (INV, UNS, INV)
    rc, p = plan(good, 65, 33, 32)
    assert rc == UNS and p.param_count > 0


# ---- the restatement against torch.nn.functional

def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_ops_against_torch():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x = rng.normal(size=(2, 6, 5, 7))
    for k, stride, groups, cout in ((1, 1, 1, 5), (3, 1, 1, 4), (3, 2, 1, 4), (3, 1, 6, 6), (3, 2, 6, 6)):
        w = rng.normal(size=(cout, 6 // groups, k, k))
        want = F.conv2d(t(x), t(w), None, stride, (k - 1) // 2, 1, groups).numpy()
        got = R.conv2d(x, w, stride, (k - 1) // 2, groups)
        assert got.shape == want.shape and _rel(got, want) <= 1e-12, (k, stride, groups)
    for shape in ((1, 2, 1, 1), (1, 2, 2, 2), (2, 3, 5, 7)):
        x = rng.normal(size=shape) - 4.0
        for k in R.SPP_POOLING:
            want = F.max_pool2d(t(x), k, 1, k // 2).numpy()
            assert (R.max_pool(x, k) == want).all(), (shape, k)
        assert (R.upsample2(x) == F.interpolate(t(x), scale_factor=2, mode="nearest").numpy()).all()
    g, b, m, v = rng.uniform(0.8, 1.2, 6), rng.normal(size=6), rng.normal(size=6), rng.uniform(0.5, 1.5, 6)
    x = rng.normal(size=(2, 6, 5, 7))
    want = F.batch_norm(t(x), t(m), t(v), t(g), t(b), False, 0.03, R.BN_EPS).numpy()
    assert _rel(R.batch_norm(x, g, b, m, v), want) <= 1e-12
    assert _rel(R.silu(x), F.silu(t(x)).numpy()) <= 1e-12


def test_whole_tiny_net_against_torch():
    """The model written a third time, on torch.nn.functional, from the same model files: one tiny net at 32 x 32 in f64."""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    case = K.Case("tiny", 3, 32, 32, 3)
    P = {k: torch.from_numpy(v.astype(np.float64)) for k, v in case.P.items()}
    width, depth, dw = 0.375, 0.33, False

    def base(n, x, k=1, s=1, groups=1):
        y = F.conv2d(x, P[n + ".conv.weight"], None, s, (k - 1) // 2, 1, groups)
        return F.silu(F.batch_norm(y, P[n + ".bn.running_mean"], P[n + ".bn.running_var"], P[n + ".bn.weight"], P[n + ".bn.bias"], False, 0.03, 1e-3))

    def conv(n, x, k, s):
        return base(n + ".pconv", base(n + ".dconv", x, k, s, x.shape[1])) if dw else base(n, x, k, s)

    def c3(n, x, blocks, shortcut):
        x1, x2 = base(n + ".conv1", x), base(n + ".conv2", x)
        for i in range(blocks):
            y = conv("%s.m.%d.conv2" % (n, i), base("%s.m.%d.conv1" % (n, i), x1), 3, 1)
            x1 = y + x1 if shortcut else y
        return base(n + ".conv3", torch.cat([x1, x2], 1))

    def dark(n, x, blocks, spp):
        x = conv(n + ".conv", x, 3, 2)
        if spp:
            x = base(n + ".spp.conv1", x)
            x = base(n + ".spp.conv2", torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1))
        return c3(n + ".c3", x, blocks, not spp)

    up = lambda x: F.interpolate(x, scale_factor=2, mode="nearest")
    x = torch.from_numpy(R.input_tensor(case.frames).astype(np.float64))
    x = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
    bb = "backbone.backbone."
    x = dark(bb + "dark2", base(bb + "stem.conv", x, 3, 1), 1, False)
    f0 = dark(bb + "dark3", x, 3, False)
    f1 = dark(bb + "dark4", f0, 3, False)
    f2 = dark(bb + "dark5", f1, 1, True)
    fpn0 = base("backbone.lateral_conv0", f2)
    fo0 = c3("backbone.c3_p4", torch.cat([up(fpn0), f1], 1), 1, False)
    fpn1 = base("backbone.reduce_conv1", fo0)
    pan2 = c3("backbone.c3_p3", torch.cat([up(fpn1), f0], 1), 1, False)
    pan1 = c3("backbone.c3_n3", torch.cat([conv("backbone.bu_conv2", pan2, 3, 2), fpn1], 1), 1, False)
    pan0 = c3("backbone.c3_n4", torch.cat([conv("backbone.bu_conv1", pan1, 3, 2), fpn0], 1), 1, False)
    want = []
    for i, feat in enumerate((pan2, pan1, pan0)):
        feat = base("head.stems.%d" % i, feat)
        branch = lambda b: conv("head.%s_convs.%d.conv1" % (b, i), conv("head.%s_convs.%d.conv0" % (b, i), feat, 3, 1), 3, 1)
        pred = lambda b, y: F.conv2d(y, P["head.%s_preds.%d.weight" % (b, i)], P["head.%s_preds.%d.bias" % (b, i)])
        cf, rf = branch("cls"), branch("reg")
        want.append(torch.cat([pred("reg", rf), pred("obj", rf), pred("cls", cf)], 1).numpy())
    got = case.ref(np.float64)
    assert (depth, width) == K.CONFIGS["tiny"][:2]
    for l in range(3):
        assert got[l].shape == want[l].shape and _rel(got[l], want[l]) <= 1e-12, (l, _rel(got[l], want[l]))
