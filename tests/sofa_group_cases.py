"""Member shapes, seeded block streams and filter schedules for the sofalizer group tests (tests/test_gpu_agroup_sofa.py,
tests/test_gpu_agroup_sofa_lifecycle.py, tests/test_agroup_sofa_cpu.py) and for the lone-path guard (tools/sofa_lone_crc.py writes
tests/golden/sofa_lone_crc.json from the same schedules).

Everything is generated from seeds; nothing is read."""
import os
import zlib

import numpy as np

import audio_state_cases as A

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CRC_FIXTURE = os.path.join(GOLDEN_DIR, "sofa_lone_crc.json")

# (channels, filter length L, partition-length P, block-length B): the members of the heterogeneous set
SHAPES = [
    (2, 20, 8, 8),          # smallest P: 8 butterflies per stage on 256 lanes
    (1, 33, 16, 64),        # K = 3, B / P = 4
    (3, 64, 64, 64),        # L = P: one partition
    (2, 17, 16, 48),        # L = P + 1; sub-blocks per block coprime to K
    (6, 128, 64, 256),      # channel 3 dropped; the element's default geometry
    (64, 40, 16, 32),       # most channels
    (2, 200, 64, 256),      # shares P = 64 with two other members
    (1, 3000, 2048, 2048),  # 112 KiB of LDS
]
DROPS = {(6, 128, 64, 256): (3,)}   # LFE1 of a 5.1 layout: ChannelProcessor::Drop


def key(shape):
    return "C%d_L%d_P%d_B%d" % tuple(shape)


def guard_shapes():
    """the shapes of the lone-path guard: the heterogeneous set, then what audio_state_cases.SOFA_NEW_SHAPES adds to it"""
    out = list(SHAPES)
    for s in A.SOFA_NEW_SHAPES:
        if s not in out:
            out.append(s)
    return out


def partitions(shape):
    _, L, P, _ = shape
    return -(-L // P)


def n_blocks(shape):
    """blocks that make at least 2K + 1 sub-blocks (every delay-line slot wraps), four at the least"""
    _, _, P, B = shape
    return max(4, -(-(2 * partitions(shape) + 1) // (B // P)))


def schedule(shape, seed=0, blocks=None):
    """{"drops": channels, "filters": [(channel, left, right, delay_left, delay_right)] set before the first block,
    "blocks": [(x [B][C] f32, gains [C] f32, [filters set before this block])]}: noise, gains that move with every block, the filter of
    the last undropped channel replaced half way"""
    C, L, P, B = shape
    nb = n_blocks(shape) if blocks is None else blocks
    rng = np.random.default_rng(104729 * C + 7919 * L + 31 * P + B + 1000003 * seed)
    drops = tuple(DROPS.get(tuple(shape), ()))
    live = [c for c in range(C) if c not in drops]
    flt = A.sofa_filters(rng, C, L)
    filters = [(c, flt[c][0], flt[c][1], c % 3, (2 * c) % 5) for c in live]
    out = []
    for b in range(nb):
        x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
        for c in drops:
            x[:, c] = 100.0   # whatever a dropped channel carries must not reach the output
        gains = rng.uniform(0.2, 1.0, C).astype(np.float32)
        changes = []
        if b == nb // 2:
            l2, r2 = A.sofa_filters(rng, 1, L)[0]
            changes.append((live[-1], l2, r2, 0, 1))
        out.append((x, gains, changes))
    return {"drops": drops, "filters": filters, "blocks": out}


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def lone_context(mi355fx, shape, sched):
    """a lone Context set up as the member: geometry, drop flags, the filters of before the first block"""
    ctx = mi355fx.Context(0)
    ctx.sofa_setup(*shape)
    for c in sched["drops"]:
        ctx.sofa_set_drop(c)
    for f in sched["filters"]:
        ctx.sofa_set_filter(*f)
    return ctx


def lone_outputs(mi355fx, shape, sched):
    """the [B][2] f32 output of every block of the schedule through a lone Context"""
    ctx = lone_context(mi355fx, shape, sched)
    try:
        outs = []
        for (x, gains, changes) in sched["blocks"]:
            for f in changes:
                ctx.sofa_set_filter(*f)
            outs.append(np.array(ctx.sofa_process_block(x, gains), np.float32).reshape(-1, 2).copy())
        return outs
    finally:
        ctx.close()


def lone_crcs(mi355fx, shape):
    return [crc(o) for o in lone_outputs(mi355fx, shape, schedule(shape))]


# What the first guard does not reach, recorded later than the rest, at the commit the entry names (the "extra" section of
# the fixture): a reset with a filter set behind it, two set_filter calls on one channel before the first block, and the device
# entry point. n_blocks(shape) blocks each.
EXTRA_SHAPES = [(2, 20, 8, 8), (2, 17, 16, 48), (6, 128, 64, 256)]


def lone_reset_outputs(mi355fx, shape):
    """schedule(shape) through the host entry point, with two additions: the first live channel's filter is set twice before the first
    block (another pair first, the scheduled one last: only the last may count), and after the second block the context is reset
    and that channel gets a third pair before the next block"""
    sched = schedule(shape)
    C, L, _, _ = shape
    rng = np.random.default_rng(15485863 + 31 * C + L)
    (la, ra), (lb, rb) = A.sofa_filters(rng, 2, L)
    first = sched["filters"][0]
    ctx = lone_context(mi355fx, shape, sched)
    try:
        ctx.sofa_set_filter(first[0], la, ra, 2, 3)
        ctx.sofa_set_filter(*first)
        outs = []
        for b, (x, gains, changes) in enumerate(sched["blocks"]):
            if b == 2:
                ctx.sofa_reset()
                ctx.sofa_set_filter(first[0], lb, rb, 1, 0)
            for f in changes:
                ctx.sofa_set_filter(*f)
            outs.append(np.array(ctx.sofa_process_block(x, gains), np.float32).reshape(-1, 2).copy())
        return outs
    finally:
        ctx.close()


def lone_device_outputs(mi355fx, shape):
    """schedule(shape) through sofa_process_block_device on buffers the caller uploads and downloads itself"""
    sched = schedule(shape)
    C, _, _, B = shape
    ctx = lone_context(mi355fx, shape, sched)
    d_in, d_out = ctx.alloc(B * C * 4), ctx.alloc(B * 8)
    try:
        outs = []
        for (x, gains, changes) in sched["blocks"]:
            for f in changes:
                ctx.sofa_set_filter(*f)
            ctx.h2d(d_in, np.ascontiguousarray(x, np.float32))
            ctx.synchronize()
            ctx.sofa_process_block_device(d_in, d_out, gains)   # (returns with d_out written)
            out = np.zeros((B, 2), np.float32)
            ctx.d2h(out, d_out)
            outs.append(out)
        return outs
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
        ctx.close()


def lone_extra_crcs(mi355fx, shape):
    return {"reset": [crc(o) for o in lone_reset_outputs(mi355fx, shape)], "device": [crc(o) for o in lone_device_outputs(mi355fx, shape)]}


def join(g, i, shape, sched):
    """member i of group g set up as lone_context sets a Context up"""
    g.sofa_setup(i, *shape)
    for c in sched["drops"]:
        g.sofa_set_drop(i, c)
    for f in sched["filters"]:
        g.sofa_set_filter(i, *f)


def same(got, want, what=None):
    """bit for bit: the bodies of the kernels are shared, there is no tolerance"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]), float(np.abs(got - want).max()))


def expected_launches(shapes, pending_members):
    """launches of one launch set of the members `shapes` [(C, L, P, B)], of which those at the indices `pending_members` have a filter
    pending: one per distinct partition length among the pending filters, one per distinct partition length among the members, one mix"""
    return len({shapes[i][2] for i in pending_members}) + len({s[2] for s in shapes}) + 1
