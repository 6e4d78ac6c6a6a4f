"""sofalizer's per-block loop on the device (uniformly partitioned FFT convolution in LDS, csrc/sofa_kernels.hip) through the
C ABI against the time-domain oracle (oracle.SofaRenderer). The crate that does this in the reference (sofar) is not in the
reference tree: parity is that of a streaming linear convolution, tolerance 2e-6 of full scale.

Shapes beyond those the 2e-6 rule was written for (partitions of 8 and of 512 .. 2048, one partition, 64 channels) are held to
TWICE the error of a numpy float32 restatement of the same algorithm (audio_state_cases.SofaF32: complex64 radix-2 transforms)
against the same f64 oracle on the same run - two f32 transforms of one length that differ in butterfly order and twiddle
source can each be off by that much in opposite directions. Measured on the CPU (worst |f32 - f64| / max(1, max|f64|) over
audio_state_cases.sofa_run; tests/test_audio_state_cpu.py recomputes every figure):

    channels  L     P     B      f32 restatement   device bound (x2)   the 2e-6 * max(1, L // 64) rule would allow
    2         20    8     8      1.14e-7           2.28e-7             2.0e-6
    2         50    8     64     2.04e-7           4.08e-7             2.0e-6
    2         1500  512   512    2.06e-7           4.12e-7             4.6e-5
    1         1024  512   1024   2.18e-7           4.36e-7             3.2e-5
    1         2048  1024  1024   2.11e-7           4.22e-7             6.4e-5
    2         1024  1024  2048   2.43e-7           4.86e-7             3.2e-5
    1         3000  2048  2048   2.06e-7           4.12e-7             9.2e-5
    2         2049  2048  4096   2.37e-7           4.74e-7             6.4e-5
    2         10    16    32     1.67e-7           3.34e-7             2.0e-6
    2         16    16    16     1.64e-7           3.28e-7             2.0e-6
    2         17    16    48     1.35e-7           2.70e-7             2.0e-6
    64        40    16    32     2.45e-7           4.90e-7             2.0e-6
    2         80    16    48     2.43e-7           4.86e-7             2.0e-6
"""
import numpy as np
import pytest

import audio_state_cases as A

pytestmark = pytest.mark.gpu
TOL = 2e-6


def _filters(rng, channels, L):
    k = np.arange(L)
    out = []
    for c in range(channels):
        env = np.exp(-k / (0.1 * L + 4.0))
        out.append(((0.5 * env * rng.standard_normal(L)).astype(np.float32), (0.4 * env * rng.standard_normal(L)).astype(np.float32)))
    return out


@pytest.mark.parametrize("channels,L,P,B", [(2, 200, 64, 256), (6, 512, 64, 256), (1, 33, 16, 64), (8, 1024, 128, 512), (3, 64, 64, 64), (2, 2048, 256, 256)])
def test_sofalizer_blocks_match_time_domain_convolution(ctx, oracle, channels, L, P, B):
    rng = np.random.default_rng(channels * 1000 + L)
    flt = _filters(rng, channels, L)
    ref = oracle.SofaRenderer(channels, L, B)
    ctx.sofa_setup(channels, L, P, B)
    for c, (l, r) in enumerate(flt):
        d = (c % 3, (2 * c) % 5)
        ctx.sofa_set_filter(c, l, r, *d)
        ref.set_filter(c, l, r, *d)
    gains = (0.5 + 0.5 * rng.random(channels)).astype(np.float32)
    worst = 0.0
    for blk in range(7):
        x = (0.5 * rng.standard_normal((B, channels))).astype(np.float32)
        if blk == 3:   # a source moves: new filter from this block on (State::update_filters, sofa/imp.rs:129-160)
            l2, r2 = _filters(rng, 1, L)[0]
            ctx.sofa_set_filter(0, l2, r2, 1, 0)
            ref.set_filter(0, l2, r2, 1, 0)
        got, exp = ctx.sofa_process_block(x, gains), ref.process_block(x, gains)
        worst = max(worst, float(np.abs(got - exp).max()))
    scale = max(1.0, float(np.abs(exp).max()))
    assert worst <= TOL * scale * max(1, L // 64), (worst, scale)


class _Device:
    """the context behind the interface audio_state_cases.sofa_run drives"""

    def __init__(self, ctx, channels, L, P, B):
        self.ctx = ctx
        ctx.sofa_setup(channels, L, P, B)

    def set_filter(self, *a):
        self.ctx.sofa_set_filter(*a)

    def process_block(self, x, gains):
        return self.ctx.sofa_process_block(x, gains)


@pytest.mark.parametrize("shape", A.SOFA_NEW_SHAPES, ids=["-".join(map(str, s)) for s in A.SOFA_NEW_SHAPES])
def test_sofalizer_partition_extremes_within_twice_the_f32_restatement(ctx, oracle, shape):
    """P = 8 (8 butterflies per stage on a 256-lane block) to P = 2048 (112 KiB of LDS), one partition with L < P, L == P and
    L == P + 1, 64 channels, sub-blocks per block coprime to the slot count; at least 2K sub-blocks, one filter replaced half way"""
    worst, scale = A.sofa_run(shape, lambda *s: _Device(ctx, *s))
    print("sofalizer %s: device error %.3g of scale %.3g, bound %.3g" % (shape, worst / scale, scale, 2.0 * A.SOFA_F32_ERR[shape]))
    assert worst <= 2.0 * A.SOFA_F32_ERR[shape] * scale, (shape, worst / scale, A.SOFA_F32_ERR[shape])


def test_sofalizer_lfe_channels_are_dropped_and_reset_clears_history(ctx, oracle):
    rng = np.random.default_rng(3)
    C, L, P, B = 6, 128, 64, 256
    flt = _filters(rng, C, L)
    ref = oracle.SofaRenderer(C, L, B)
    ctx.sofa_setup(C, L, P, B)
    for c, (l, r) in enumerate(flt):
        if c == 3:   # LFE1: ChannelProcessor::Drop, never gets a filter (sofa/imp.rs:808-821)
            ctx.sofa_set_drop(c)
            ref.drop[c] = True
            continue
        ctx.sofa_set_filter(c, l, r)
        ref.set_filter(c, l, r)
    g = np.ones(C, np.float32)
    x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
    x[:, 3] = 100.0   # whatever the LFE carries must not reach the output
    for _ in range(2):
        got, exp = ctx.sofa_process_block(x, g), ref.process_block(x, g)
        assert np.abs(got - exp).max() <= TOL * max(1.0, np.abs(exp).max())
    ctx.sofa_reset()
    ref.reset()
    z = np.zeros((B, C), np.float32)
    assert (ctx.sofa_process_block(z, g) == 0).all()   # no tail of the earlier blocks after a flush


def test_sofalizer_argument_errors(ctx):
    import mi355fx
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.sofa_setup(2, 128, 64, 200)          # "Block Length is not multiple of Partition Length" (sofa/imp.rs:775-781)
    assert e.value.status == mi355fx.ERR_INVALID_ARG and "multiple of Partition Length" in str(e.value)
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.sofa_setup(2, 128, 48, 96)           # not a power of two
    assert e.value.status == mi355fx.ERR_UNSUPPORTED
    ctx.sofa_setup(2, 16, 16, 32)
    with pytest.raises(mi355fx.Mi355Error) as e:  # channel 1 has no filter and is not dropped
        ctx.sofa_set_filter(0, np.ones(16, np.float32), np.ones(16, np.float32))
        ctx.sofa_process_block(np.zeros((32, 2), np.float32), np.ones(2, np.float32))
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED
    ctx.sofa_teardown()
