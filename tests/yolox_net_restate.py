"""A numpy restatement of yoloxinference's network, written from the model files of the reference
(analytics/burn/src/yoloxinference/yolox_burn/model/{blocks,bottleneck,darknet,pafpn,head,yolox}.rs), module by module, NOT from
csrc/yolox_net.hip. The dtype is a parameter: float64 is the checker, float32 the yardstick for f32 rounding noise.
Tensors are [N, C, H, W]. The forward stops where mi355_yolox_net_forward_device stops: per level the raw maps
cat([reg_out, obj_out, cls_out], 1) of head.rs:75 WITHOUT its two sigmoids and without Head::decode.

Parameters are enumerated in the order the structs declare their fields, named as the state dict is after the key remapping of
yolox.rs:255-272 (the enum Conv adds no path segment: a depthwise Conv is `.dconv` / `.pconv`)."""
import numpy as np

BN_EPS = 1e-3          # blocks.rs:114
SPP_POOLING = (5, 9, 13)   # bottleneck.rs:9
STRIDES = (8, 16, 32)      # head.rs:16
DEPTHS, WIDTHS = (0.33, 0.67, 1.0, 1.33), (0.25, 0.375, 0.5, 0.75, 1.0, 1.25)   # darknet.rs:51-59


def expand(num_channels, factor):
    """blocks.rs:12"""
    return int(np.floor(float(num_channels) * float(factor)))


def rust_round(v):
    """f64::round: half away from zero"""
    return int(np.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))


def base_depth(depth):
    """darknet.rs:62"""
    return max(rust_round(depth * 3.0), 1)


def num_blocks(depth):
    """pafpn.rs:106"""
    return rust_round(3.0 * depth)


# ---- the tensor operations

def conv2d(x, w, stride=1, pad=0, groups=1, bias=None):
    """Conv2d with zero padding; w [Cout, Cin / groups, k, k]; im2col + matmul in x's dtype."""
    dt = x.dtype
    w = w.astype(dt)
    n, cin, h, wd = x.shape
    cout, cg, k, _ = w.shape
    assert cin == cg * groups and cout % groups == 0
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = np.zeros((n, cin, h + 2 * pad, wd + 2 * pad), dt)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    cols = np.empty((n, cin, k, k, ho, wo), dt)
    for dy in range(k):
        for dx in range(k):
            cols[:, :, dy, dx] = xp[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
    out = np.empty((n, cout, ho, wo), dt)
    og = cout // groups
    for g in range(groups):
        a = w[g * og:(g + 1) * og].reshape(og, cg * k * k)
        b = cols[:, g * cg:(g + 1) * cg].reshape(n, cg * k * k, ho * wo)
        out[:, g * og:(g + 1) * og] = np.matmul(a, b).reshape(n, og, ho, wo)
    if bias is not None:
        out = out + bias.astype(dt).reshape(1, cout, 1, 1)
    return out


def batch_norm(x, gamma, beta, mean, var):
    """BatchNorm in inference: (x - mean) / sqrt(var + eps) * gamma + beta, in x's dtype."""
    dt = x.dtype
    r = lambda a: a.astype(dt).reshape(1, -1, 1, 1)
    return (x - r(mean)) / np.sqrt(r(var) + dt.type(BN_EPS)) * r(gamma) + r(beta)


def silu(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return x * (one / (one + np.exp(-x)))


def max_pool(x, k):
    """MaxPool2d k x k, stride 1, pad k // 2; the padding is -inf."""
    p = k // 2
    n, c, h, w = x.shape
    xp = np.full((n, c, h + 2 * p, w + 2 * p), -np.inf, x.dtype)
    xp[:, :, p:p + h, p:p + w] = x
    out = np.full_like(x, -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, xp[:, :, dy:dy + h, dx:dx + w])
    return out


def upsample2(x):
    """interpolate(.., Nearest) to twice the size: out[y][x] = in[y // 2][x // 2] (pafpn.rs:37-44)"""
    return x.repeat(2, axis=2).repeat(2, axis=3)


def focus(x):
    """blocks.rs:187-208: cat([top-left, bottom-left, top-right, bottom-right], 1)"""
    return np.concatenate([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], axis=1)


# ---- the modules. Each declares its parameters (decl) and runs (fwd); `taps` collects every activation by name.

class BaseConv:
    """Conv2d (no bias) -> BatchNorm -> SiLU (blocks.rs:76-127)"""

    def __init__(self, name, cin, cout, k, stride, groups=1):
        self.name, self.cin, self.cout, self.k, self.stride, self.groups = name, cin, cout, k, stride, groups

    def decl(self, out):
        out.append((self.name + ".conv.weight", (self.cout, self.cin // self.groups, self.k, self.k)))
        for f in ("weight", "bias", "running_mean", "running_var"):
            out.append((self.name + ".bn." + f, (self.cout,)))

    def fwd(self, P, x, taps):
        n = self.name
        y = conv2d(x, P[n + ".conv.weight"], self.stride, (self.k - 1) // 2, self.groups)
        y = silu(batch_norm(y, P[n + ".bn.weight"], P[n + ".bn.bias"], P[n + ".bn.running_mean"], P[n + ".bn.running_var"]))
        if taps is not None:
            taps[n] = y
        return y


class DwsConv:
    """blocks.rs:132-168"""

    def __init__(self, name, cin, cout, k, stride):
        self.dconv = BaseConv(name + ".dconv", cin, cin, k, stride, cin)
        self.pconv = BaseConv(name + ".pconv", cin, cout, 1, 1)

    def decl(self, out):
        self.dconv.decl(out)
        self.pconv.decl(out)

    def fwd(self, P, x, taps):
        return self.pconv.fwd(P, self.dconv.fwd(P, x, taps), taps)


def Conv(name, cin, cout, k, stride, depthwise):
    """blocks.rs:48-71"""
    return DwsConv(name, cin, cout, k, stride) if depthwise else BaseConv(name, cin, cout, k, stride)


class Bottleneck:
    """bottleneck.rs:13-65"""

    def __init__(self, name, cin, cout, shortcut, depthwise):
        self.conv1 = BaseConv(name + ".conv1", cin, cout, 1, 1)
        self.conv2 = Conv(name + ".conv2", cout, cout, 3, 1, depthwise)
        self.shortcut, self.name = shortcut, name

    def decl(self, out):
        self.conv1.decl(out)
        self.conv2.decl(out)

    def fwd(self, P, x, taps):
        y = self.conv2.fwd(P, self.conv1.fwd(P, x, taps), taps)
        if self.shortcut:
            y = y + x
            if taps is not None:
                taps[self.name + "+x"] = y
        return y


class SppBottleneck:
    """bottleneck.rs:69-129"""

    def __init__(self, name, cin, cout):
        hidden = cin // 2
        self.conv1 = BaseConv(name + ".conv1", cin, hidden, 1, 1)
        self.conv2 = BaseConv(name + ".conv2", hidden * 4, cout, 1, 1)

    def decl(self, out):
        self.conv1.decl(out)
        self.conv2.decl(out)

    def fwd(self, P, x, taps):
        x = self.conv1.fwd(P, x, taps)
        return self.conv2.fwd(P, np.concatenate([x] + [max_pool(x, k) for k in SPP_POOLING], axis=1), taps)


class CspBottleneck:
    """bottleneck.rs:134-206"""

    def __init__(self, name, cin, cout, n, expansion, shortcut, depthwise):
        hidden = expand(cout, expansion)
        self.conv1 = BaseConv(name + ".conv1", cin, hidden, 1, 1)
        self.conv2 = BaseConv(name + ".conv2", cin, hidden, 1, 1)
        self.conv3 = BaseConv(name + ".conv3", 2 * hidden, cout, 1, 1)
        self.m = [Bottleneck("%s.m.%d" % (name, i), hidden, hidden, shortcut, depthwise) for i in range(n)]

    def decl(self, out):
        for mod in [self.conv1, self.conv2, self.conv3] + self.m:
            mod.decl(out)

    def fwd(self, P, x, taps):
        x1, x2 = self.conv1.fwd(P, x, taps), self.conv2.fwd(P, x, taps)
        for b in self.m:
            x1 = b.fwd(P, x1, taps)
        return self.conv3.fwd(P, np.concatenate([x1, x2], axis=1), taps)


class CspBlock:
    """darknet.rs:118-172: fields conv, c3, spp; forward conv, spp, c3"""

    def __init__(self, name, cin, cout, depth, spp, depthwise):
        self.conv = Conv(name + ".conv", cin, cout, 3, 2, depthwise)
        self.c3 = CspBottleneck(name + ".c3", cout, cout, depth, 0.5, not spp, depthwise)
        self.spp = SppBottleneck(name + ".spp", cout, cout) if spp else None

    def decl(self, out):
        self.conv.decl(out)
        self.c3.decl(out)
        if self.spp:
            self.spp.decl(out)

    def fwd(self, P, x, taps):
        x = self.conv.fwd(P, x, taps)
        if self.spp:
            x = self.spp.fwd(P, x, taps)
        return self.c3.fwd(P, x, taps)


class CspDarknet:
    """darknet.rs:19-113"""

    def __init__(self, name, depth, width, depthwise):
        assert depth in DEPTHS and width in WIDTHS
        bc, bd = expand(64, width), base_depth(depth)
        self.stem = BaseConv(name + ".stem.conv", 3 * 4, bc, 3, 1)   # Focus holds one BaseConv named `conv`
        self.dark2 = CspBlock(name + ".dark2", bc, bc * 2, bd, False, depthwise)
        self.dark3 = CspBlock(name + ".dark3", bc * 2, bc * 4, bd * 3, False, depthwise)
        self.dark4 = CspBlock(name + ".dark4", bc * 4, bc * 8, bd * 3, False, depthwise)
        self.dark5 = CspBlock(name + ".dark5", bc * 8, bc * 16, bd, True, depthwise)

    def decl(self, out):
        for mod in (self.stem, self.dark2, self.dark3, self.dark4, self.dark5):
            mod.decl(out)

    def fwd(self, P, x, taps):
        x = self.stem.fwd(P, focus(x), taps)
        x = self.dark2.fwd(P, x, taps)
        f1 = self.dark3.fwd(P, x, taps)
        f2 = self.dark4.fwd(P, f1, taps)
        f3 = self.dark5.fwd(P, f2, taps)
        return f1, f2, f3


class Pafpn:
    """pafpn.rs:23-176"""

    def __init__(self, name, depth, width, depthwise):
        hidden = [expand(2 * 256, width), expand(2 * 512, width)]
        ch = [expand(256, width), expand(512, width), expand(1024, width)]
        n = num_blocks(depth)
        self.backbone = CspDarknet(name + ".backbone", depth, width, depthwise)
        self.lateral_conv0 = BaseConv(name + ".lateral_conv0", ch[2], ch[1], 1, 1)
        self.c3_n3 = CspBottleneck(name + ".c3_n3", hidden[0], ch[1], n, 0.5, False, depthwise)
        self.c3_n4 = CspBottleneck(name + ".c3_n4", hidden[1], ch[2], n, 0.5, False, depthwise)
        self.c3_p3 = CspBottleneck(name + ".c3_p3", hidden[0], ch[0], n, 0.5, False, depthwise)
        self.c3_p4 = CspBottleneck(name + ".c3_p4", hidden[1], ch[1], n, 0.5, False, depthwise)
        self.reduce_conv1 = BaseConv(name + ".reduce_conv1", ch[1], ch[0], 1, 1)
        self.bu_conv1 = Conv(name + ".bu_conv1", ch[1], ch[1], 3, 2, depthwise)
        self.bu_conv2 = Conv(name + ".bu_conv2", ch[0], ch[0], 3, 2, depthwise)

    def decl(self, out):
        for mod in (self.backbone, self.lateral_conv0, self.c3_n3, self.c3_n4, self.c3_p3, self.c3_p4, self.reduce_conv1, self.bu_conv1, self.bu_conv2):
            mod.decl(out)

    def fwd(self, P, x, taps):
        f0, f1, f2 = self.backbone.fwd(P, x, taps)
        fpn_out0 = self.lateral_conv0.fwd(P, f2, taps)
        f_out0 = self.c3_p4.fwd(P, np.concatenate([upsample2(fpn_out0), f1], axis=1), taps)
        fpn_out1 = self.reduce_conv1.fwd(P, f_out0, taps)
        pan_out2 = self.c3_p3.fwd(P, np.concatenate([upsample2(fpn_out1), f0], axis=1), taps)
        p_out1 = np.concatenate([self.bu_conv2.fwd(P, pan_out2, taps), fpn_out1], axis=1)
        pan_out1 = self.c3_n3.fwd(P, p_out1, taps)
        p_out0 = np.concatenate([self.bu_conv1.fwd(P, pan_out1, taps), fpn_out0], axis=1)
        pan_out0 = self.c3_n4.fwd(P, p_out0, taps)
        return pan_out2, pan_out1, pan_out0


class Pred:
    """a prediction layer: Conv2d 1 x 1 with bias (head.rs:157-165)"""

    def __init__(self, name, cin, cout):
        self.name, self.cin, self.cout = name, cin, cout

    def decl(self, out):
        out.append((self.name + ".weight", (self.cout, self.cin, 1, 1)))
        out.append((self.name + ".bias", (self.cout,)))

    def fwd(self, P, x, taps):
        return conv2d(x, P[self.name + ".weight"], 1, 0, 1, P[self.name + ".bias"])


class ConvBlock:
    """blocks.rs:237-271"""

    def __init__(self, name, ch, depthwise):
        self.conv0, self.conv1 = Conv(name + ".conv0", ch, ch, 3, 1, depthwise), Conv(name + ".conv1", ch, ch, 3, 1, depthwise)

    def decl(self, out):
        self.conv0.decl(out)
        self.conv1.decl(out)

    def fwd(self, P, x, taps):
        return self.conv1.fwd(P, self.conv0.fwd(P, x, taps), taps)


class Head:
    """head.rs:38-191, up to the raw maps"""

    def __init__(self, name, num_classes, width, depthwise):
        hc = expand(256, width)
        self.stems = [BaseConv("%s.stems.%d" % (name, i), expand(c, width), hc, 1, 1) for i, c in enumerate((256, 512, 1024))]
        self.cls_convs = [ConvBlock("%s.cls_convs.%d" % (name, i), hc, depthwise) for i in range(3)]
        self.reg_convs = [ConvBlock("%s.reg_convs.%d" % (name, i), hc, depthwise) for i in range(3)]
        self.cls_preds = [Pred("%s.cls_preds.%d" % (name, i), hc, num_classes) for i in range(3)]
        self.reg_preds = [Pred("%s.reg_preds.%d" % (name, i), hc, 4) for i in range(3)]
        self.obj_preds = [Pred("%s.obj_preds.%d" % (name, i), hc, 1) for i in range(3)]

    def decl(self, out):
        for group in (self.stems, self.cls_convs, self.reg_convs, self.cls_preds, self.reg_preds, self.obj_preds):
            for mod in group:
                mod.decl(out)

    def fwd(self, P, feats, taps):
        outs = []
        for i, feat in enumerate(feats):
            feat = self.stems[i].fwd(P, feat, taps)
            cls_out = self.cls_preds[i].fwd(P, self.cls_convs[i].fwd(P, feat, taps), taps)
            reg_feat = self.reg_convs[i].fwd(P, feat, taps)
            reg_out, obj_out = self.reg_preds[i].fwd(P, reg_feat, taps), self.obj_preds[i].fwd(P, reg_feat, taps)
            outs.append(np.concatenate([reg_out, obj_out, cls_out], axis=1))
        return outs


class Yolox:
    """yolox.rs:19-28, :281-302"""

    def __init__(self, depth, width, depthwise, num_classes):
        self.depth, self.width, self.depthwise, self.num_classes = depth, width, bool(depthwise), num_classes
        self.backbone = Pafpn("backbone", depth, width, self.depthwise)
        self.head = Head("head", num_classes, width, self.depthwise)
        self.params = []
        self.backbone.decl(self.params)
        self.head.decl(self.params)

    def param_floats(self):
        return sum(int(np.prod(shape)) for _, shape in self.params)

    def forward(self, P, x, dtype=np.float64, taps=None):
        """x: [N, 3, H, W] (any dtype; values are converted exactly) -> per level [N, 5 + C, h, w] raw maps in `dtype`."""
        dt = np.dtype(dtype)
        Pd = {k: np.asarray(v).astype(dt) for k, v in P.items()}
        return self.head.fwd(Pd, self.backbone.fwd(Pd, np.asarray(x).astype(dt), taps), taps)


def input_tensor(frames_u8):
    """[N, H, W, 3] u8 RGB frames -> [N, 3, H, W] float32, unscaled (yoloxinference/imp.rs:533-539)"""
    return np.ascontiguousarray(np.asarray(frames_u8).transpose(0, 3, 1, 2)).astype(np.float32)
