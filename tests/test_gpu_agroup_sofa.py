"""sofalizer through an audio group (csrc/agroup.hip kind `sofa`, csrc/sofa_kernels.hip job tables): a member's output against a lone
Context given the same setup, filters, drops, gains and blocks. The kernels' bodies are shared between the two forms, so the
comparison is numpy.array_equal on float32: there is no tolerance anywhere but in the oracle test, whose bound is
tests/test_gpu_sofa.py's. The lone path itself is pinned by CRC-32s taken before the bodies were moved
(tests/golden/sofa_lone_crc.json, tools/sofa_lone_crc.py)."""
import json

import numpy as np
import pytest

import audio_state_cases as A
import mi355fx
import sofa_group_cases as S

pytestmark = pytest.mark.gpu

UNIFORM = (2, 128, 64, 256)


def _raises(status, fn, *a, **kw):
    with pytest.raises(mi355fx.Mi355Error) as e:
        fn(*a, **kw)
    assert e.value.status == status, (e.value.status, str(e.value))
    return str(e.value)


def _filters(seed, shape):
    C, L, _, _ = shape
    return A.sofa_filters(np.random.default_rng(seed), C, L)


def _noise(seed, frames, channels):
    return (0.5 * np.random.default_rng(seed).standard_normal((frames, channels))).astype(np.float32)


def _block(g, i, x, gains, n_blocks=1):
    """one member alone in its launch set (linger 0: its wait runs the set of whoever is there)"""
    frames = g.wait(g.submit_sofa(i, x, gains, n_blocks=n_blocks))
    assert frames == x.shape[0]
    return g.sofa_output(i).copy()


# ---------------------------------------------------------------- 1: the heterogeneous set

def test_heterogeneous_set_equals_lone_contexts(mi355lib):
    """eight members, four partition lengths, every launch set holds all of them; 7 intervals, so that the member with the most
    slots against the fewest sub-blocks per block ((2, 20, 8, 8): K = 3, one sub-block per block) runs 2K + 1 sub-blocks"""
    shapes = S.SHAPES
    ni = max(S.n_blocks(s) for s in shapes)
    assert ni == 7
    for s in shapes:
        assert ni * (s[3] // s[2]) >= 2 * S.partitions(s) + 1, s
    scheds = [S.schedule(s, seed=1, blocks=ni) for s in shapes]
    want = [S.lone_outputs(mi355fx, s, sc) for s, sc in zip(shapes, scheds)]
    g = mi355fx.AudioGroup("sofa", len(shapes))
    try:
        g.set_linger(0)
        for i, (s, sc) in enumerate(zip(shapes, scheds)):
            S.join(g, i, s, sc)
            assert g.sofa_info(i) == (S.partitions(s), 2 * s[2], s[0] - len(sc["drops"])), s
        launches = 0
        for b in range(ni):
            pending = []
            for i, sc in enumerate(scheds):
                for f in sc["blocks"][b][2]:
                    g.sofa_set_filter(i, *f)
                if g.sofa_info(i)[2]:
                    pending.append(i)
            assert pending == (list(range(len(shapes))) if b in (0, ni // 2) else []), (b, pending)
            tickets = [g.submit_sofa(i, sc["blocks"][b][0], sc["blocks"][b][1]) for i, sc in enumerate(scheds)]
            launches += S.expected_launches(shapes, pending)
            assert g.stats() == (len(shapes) * (b + 1), b + 1, len(shapes))      # the eighth submit ran the set
            assert g.sofa_launches() == launches, b
            for i, s in enumerate(shapes):
                assert g.wait(tickets[i]) == s[3]
                S.same(g.sofa_output(i), want[i][b], (s, b))
                assert g.sofa_info(i) == (S.partitions(s), 2 * s[2], 0)
        # four distinct partition lengths + the mix per set, four filter launches in the first interval and in the one after the move
        assert launches == 7 * 5 + 2 * 4
    finally:
        g.close()


# ---------------------------------------------------------------- 2: the filter queue

def test_filter_queue_replace_and_last_one_wins(mi355lib):
    shape = UNIFORM
    C, L, P, B = shape
    g = mi355fx.AudioGroup("sofa", 4)
    lone = [mi355fx.Context(0) for _ in range(4)]
    try:
        g.set_linger(0)
        for i in range(4):
            g.sofa_setup(i, *shape)
            lone[i].sofa_setup(*shape)
            for c, (l, r) in enumerate(_filters(10 + i, shape)):
                g.sofa_set_filter(i, c, l, r, c, 2 * c)
                lone[i].sofa_set_filter(c, l, r, c, 2 * c)
        gains = np.array([0.7, 0.4], np.float32)

        def interval(b, who=range(4)):
            xs = {i: _noise(100 * b + i, B, C) for i in who}
            tickets = {i: g.submit_sofa(i, xs[i], gains) for i in who}
            for i in who:
                assert g.wait(tickets[i]) == B
                S.same(g.sofa_output(i), lone[i].sofa_process_block(xs[i], gains), (b, i))

        interval(0)
        assert g.sofa_launches() == 3
        interval(1)
        assert g.sofa_launches() == 5                       # nothing pending: convolve + mix
        # a filter replaced between blocks takes effect with the member's next block
        l2, r2 = _filters(20, shape)[0]
        assert g.sofa_info(1)[2] == 0
        g.sofa_set_filter(1, 0, l2, r2, 0, 3)
        lone[1].sofa_set_filter(0, l2, r2, 0, 3)
        assert g.sofa_info(1)[2] == 1 and g.sofa_launches() == 5   # queued: nothing was launched
        interval(2)
        assert g.sofa_info(1)[2] == 0 and g.sofa_launches() == 8
        # two calls on one channel before a submit: only the last is transformed; the lone context gets only the second
        la, ra = _filters(21, shape)[1]
        lb, rb = _filters(22, shape)[1]
        g.sofa_set_filter(2, 1, la, ra, 5, 0)
        assert g.sofa_info(2)[2] == 1
        g.sofa_set_filter(2, 1, lb, rb, 0, 1)
        assert g.sofa_info(2)[2] == 1
        lone[2].sofa_set_filter(1, lb, rb, 0, 1)
        interval(3)
        assert g.sofa_info(2)[2] == 0 and g.sofa_launches() == 11
        interval(4)
        assert g.sofa_launches() == 13
    finally:
        g.close()
        for c in lone:
            c.close()


def test_filter_of_a_member_that_sits_out_stays_pending(mi355lib):
    shape = UNIFORM
    C, L, P, B = shape
    g = mi355fx.AudioGroup("sofa", 4)
    lone = [mi355fx.Context(0) for _ in range(4)]
    try:
        g.set_linger(0)
        for i in range(4):
            g.sofa_setup(i, *shape)
            lone[i].sofa_setup(*shape)
        # the first submit without filters
        x = _noise(1, B, C)
        gains = np.ones(C, np.float32)
        assert "no filter" in _raises(mi355fx.ERR_NOT_CONFIGURED, g.submit_sofa, 0, x, gains)
        g.sofa_set_filter(0, 0, *_filters(30, shape)[0])
        _raises(mi355fx.ERR_NOT_CONFIGURED, g.submit_sofa, 0, x, gains)      # channel 1 still has none
        assert g.stats() == (0, 0, 0)
        for i in range(4):
            for c, (l, r) in enumerate(_filters(30 + i, shape)):
                g.sofa_set_filter(i, c, l, r)
                lone[i].sofa_set_filter(c, l, r)

        def interval(b, who):
            xs = {i: _noise(100 * b + i, B, C) for i in who}
            tickets = {i: g.submit_sofa(i, xs[i], gains) for i in who}
            for i in who:
                assert g.wait(tickets[i]) == B
                S.same(g.sofa_output(i), lone[i].sofa_process_block(xs[i], gains), (b, i))

        interval(0, range(4))
        l2, r2 = _filters(40, shape)[1]
        g.sofa_set_filter(3, 1, l2, r2, 2, 2)
        lone[3].sofa_set_filter(1, l2, r2, 2, 2)
        n0 = g.sofa_launches()
        interval(1, range(3))                       # member 3 sits this one out
        assert g.sofa_launches() == n0 + 2          # no filter launch in the others' set
        assert g.sofa_info(3)[2] == 1               # ... and its filter is still pending
        assert g.stats() == (7, 2, 4)
        interval(2, range(4))                       # its next block uses it
        assert g.sofa_launches() == n0 + 2 + 3 and g.sofa_info(3)[2] == 0
        interval(3, range(4))
    finally:
        g.close()
        for c in lone:
            c.close()


# ---------------------------------------------------------------- 3: several blocks per submit

@pytest.mark.parametrize("shape", [(2, 50, 8, 64), (2, 200, 64, 256)], ids=["2-50-8-64", "2-200-64-256"])
def test_three_blocks_in_one_submit_equal_three_lone_blocks(mi355lib, shape):
    C, L, P, B = shape
    sc = S.schedule(shape, seed=3, blocks=5)
    g = mi355fx.AudioGroup("sofa", 1)
    lone = S.lone_context(mi355fx, shape, sc)
    try:
        g.set_linger(0)
        S.join(g, 0, shape, sc)
        gains = sc["blocks"][0][1]
        xs = [b[0] for b in sc["blocks"]]
        one = _block(g, 0, xs[0], gains)                         # (a block before, so that the three start at a slot other than 0)
        S.same(one, lone.sofa_process_block(xs[0], gains))
        x3 = np.concatenate(xs[1:4])
        t = g.submit_sofa(0, x3, gains, n_blocks=3)
        assert g.wait(t) == 3 * B
        got = g.sofa_output(0)
        assert got.shape == (3 * B, 2)
        want = np.concatenate([lone.sofa_process_block(x, gains) for x in xs[1:4]])
        S.same(got, want, shape)
        S.same(_block(g, 0, xs[4], gains), lone.sofa_process_block(xs[4], gains))   # what the three blocks left behind
        for n in (0, 9):
            _raises(mi355fx.ERR_INVALID_ARG, g.submit_sofa, 0, np.zeros((max(n, 1) * B, C), np.float32), gains, n_blocks=n)
        assert g.sofa_launches() == 3 + 2 + 2 and g.stats() == (3, 3, 1)
    finally:
        g.close()
        lone.close()


# ---------------------------------------------------------------- 4: partial sets and device members

def test_partial_sets_and_device_members(mi355lib):
    shape = UNIFORM
    C, L, P, B = shape
    n = 32
    g = mi355fx.AudioGroup("sofa", n)
    lone = []
    dev = mi355fx.Context(0)
    d_in, d_out = {}, {}
    try:
        g.set_linger(0)
        gains = [np.random.default_rng(500 + i).uniform(0.2, 1.0, C).astype(np.float32) for i in range(n)]
        for i in range(n):
            c = mi355fx.Context(0)
            lone.append(c)
            g.sofa_setup(i, *shape)
            c.sofa_setup(*shape)
            for ch, (l, r) in enumerate(_filters(600 + i, shape)):
                g.sofa_set_filter(i, ch, l, r, ch, 0)
                c.sofa_set_filter(ch, l, r, ch, 0)
        for i in range(0, n, 4):
            d_in[i], d_out[i] = dev.alloc(B * C * 4), dev.alloc(B * 8)

        def interval(b, who, device=()):
            xs = {i: _noise(1000 * b + i, B, C) for i in who}
            tickets = {}
            for i in who:
                if i in device:
                    dev.h2d(d_in[i], xs[i])
                    dev.synchronize()
                    tickets[i] = g.submit_sofa(i, d_in[i], gains[i], out=d_out[i])
                else:
                    tickets[i] = g.submit_sofa(i, xs[i], gains[i])
            for i in who:
                assert g.wait(tickets[i]) == B
                if i in device:
                    got = np.zeros(B * 2, np.float32)
                    dev.d2h(got, d_out[i])
                else:
                    got = g.sofa_output(i)
                S.same(got, lone[i].sofa_process_block(xs[i], gains[i]), (b, i))

        everybody, odd = list(range(n)), list(range(1, n, 2))
        interval(0, everybody)
        interval(1, odd)                                    # the even members sit out: the first wait runs the set of the 16
        interval(2, everybody)                              # ... and are bit-exact in their following block
        interval(3, everybody, device=set(range(0, n, 4)))  # every fourth member hands over device buffers
        interval(4, everybody)
        assert g.stats() == (4 * n + n // 2, 5, n)          # one launch set per interval
        assert g.sofa_launches() == 3 + 2 + 2 + 2 + 2
    finally:
        g.close()
        for p in list(d_in.values()) + list(d_out.values()):
            dev.free(p)
        dev.close()
        for c in lone:
            c.close()


# ---------------------------------------------------------------- 5: drop and reset

def test_drop_and_reset(mi355lib):
    shape = (6, 128, 64, 256)
    C, L, P, B = shape
    sc = S.schedule(shape, seed=5, blocks=4)
    assert sc["drops"] == (3,) and (sc["blocks"][0][0][:, 3] == 100.0).all()
    g = mi355fx.AudioGroup("sofa", 2)
    lone = S.lone_context(mi355fx, shape, sc)
    try:
        g.set_linger(0)
        S.join(g, 0, shape, sc)
        assert g.sofa_info(0) == (2, 128, 5)
        (x0, g0, _), (x1, g1, _), (x2, g2, ch2), (x3, g3, _) = sc["blocks"]
        got = _block(g, 0, x0, g0)
        S.same(got, lone.sofa_process_block(x0, g0))
        assert np.abs(got).max() < 20.0                    # the 100.0 of the dropped channel did not reach the output
        assert "fixed" in _raises(mi355fx.ERR_INVALID_ARG, g.sofa_set_drop, 0, 2, True)
        assert "fixed" in _raises(mi355fx.ERR_INVALID_ARG, g.sofa_set_drop, 0, 3, False)
        S.same(_block(g, 0, x1, g1), lone.sofa_process_block(x1, g1))
        # a filter set, then a reset: the pending one and the transformed ones both survive, the history does not
        g.sofa_set_filter(0, *ch2[0])
        lone.sofa_set_filter(*ch2[0])
        g.sofa_reset(0)
        lone.sofa_reset()
        assert g.sofa_info(0)[2] == 1
        z = np.zeros((B, C), np.float32)
        assert not _block(g, 0, z, g2).any()               # a zero block after the reset: exactly zero, no tail
        assert not lone.sofa_process_block(z, g2).any()
        assert g.sofa_info(0)[2] == 0
        got = _block(g, 0, x2, g2)
        assert got.any()
        S.same(got, lone.sofa_process_block(x2, g2))       # the old filters and the one that was pending at the reset apply
        g.sofa_reset(0)
        lone.sofa_reset()
        g.sofa_set_drop(0, 3, True)                        # after a reset the flags can be set again
        S.same(_block(g, 0, x3, g3), lone.sofa_process_block(x3, g3))
    finally:
        g.close()
        lone.close()


# ---------------------------------------------------------------- 6: against the oracle

class _Member:
    """member 0 of a group of one behind the interface audio_state_cases.sofa_run drives"""

    def __init__(self, g, channels, L, P, B):
        self.g = g
        g.sofa_setup(0, channels, L, P, B)

    def set_filter(self, *a):
        self.g.sofa_set_filter(0, *a)

    def process_block(self, x, gains):
        return _block(self.g, 0, x, gains)


def test_member_within_twice_the_f32_restatement_of_the_oracle(mi355lib, oracle):
    """the bound and its derivation are tests/test_gpu_sofa.py's: twice the error of the float32 restatement on the same run"""
    shape = (2, 1500, 512, 512)
    g = mi355fx.AudioGroup("sofa", 1)
    try:
        g.set_linger(0)
        worst, scale = A.sofa_run(shape, lambda *s: _Member(g, *s))
        print("sofalizer member %s: device error %.3g of scale %.3g, bound %.3g" % (shape, worst / scale, scale, 2.0 * A.SOFA_F32_ERR[shape]))
        assert worst <= 2.0 * A.SOFA_F32_ERR[shape] * scale, (shape, worst / scale, A.SOFA_F32_ERR[shape])
    finally:
        g.close()


# ---------------------------------------------------------------- 7: the lone path is what it was

@pytest.mark.parametrize("shape", S.guard_shapes(), ids=[S.key(s) for s in S.guard_shapes()])
def test_lone_path_unchanged(mi355lib, shape):
    """CRC-32 of every output block of a lone context, recorded at the commit before the kernels' bodies were shared"""
    with open(S.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert S.lone_crcs(mi355fx, shape) == doc["shapes"][S.key(shape)], shape


@pytest.mark.parametrize("shape", S.EXTRA_SHAPES, ids=[S.key(s) for s in S.EXTRA_SHAPES])
def test_lone_reset_double_set_filter_and_device_entry_unchanged(mi355lib, shape):
    """the fixture's "extra" section, recorded at the commit before audio_fft.hpp took over the two files' shared helpers: a reset after the second
    block with a filter set behind it, two set_filter calls on one channel before the first block, and the device entry point"""
    with open(S.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert S.lone_extra_crcs(mi355fx, shape) == doc["extra"]["shapes"][S.key(shape)], shape


# ---------------------------------------------------------------- 8: the life of a lone context

def _lone_run(ctx, shape, seed, blocks):
    """set `ctx` up as `shape` with seeded filters and run seeded blocks -> the outputs"""
    C, L, P, B = shape
    ctx.sofa_setup(*shape)
    for c, (l, r) in enumerate(_filters(seed, shape)):
        ctx.sofa_set_filter(c, l, r, c % 2, 1)
    gains = np.linspace(0.3, 0.9, C).astype(np.float32)
    return [ctx.sofa_process_block(_noise(seed + 1 + b, B, C), gains).copy() for b in range(blocks)]


def test_lone_context_set_up_again_equals_a_fresh_one(mi355lib):
    first, second = (2, 20, 8, 8), (1, 33, 16, 64)
    ctx, fresh = mi355fx.Context(0), mi355fx.Context(0)
    try:
        _lone_run(ctx, first, 70, 2)
        got = _lone_run(ctx, second, 80, 3)          # another geometry on the same context: nothing of the first may survive
        want = _lone_run(fresh, second, 80, 3)
        for b in range(3):
            assert got[b].shape == (64, 2) and got[b].any()
            S.same(got[b], want[b], b)
        ctx.sofa_teardown()
        assert "not configured" in _raises(mi355fx.ERR_NOT_CONFIGURED, ctx.sofa_reset)
        ctx.sofa_teardown()                           # nothing left to trip over
        S.same(_lone_run(ctx, second, 80, 1)[0], want[0])
    finally:
        ctx.close()
        ctx.close()
        fresh.close()


def test_refused_lone_block_moves_no_state(mi355lib):
    shape = (2, 17, 16, 48)
    C, L, P, B = shape
    flt = _filters(90, shape)
    gains = np.array([0.8, 0.5], np.float32)
    x = [_noise(91 + b, B, C) for b in range(2)]
    ctx, never = mi355fx.Context(0), mi355fx.Context(0)
    try:
        for c in (ctx, never):
            c.sofa_setup(*shape)
            c.sofa_set_filter(0, *flt[0])
        assert "no filter" in _raises(mi355fx.ERR_NOT_CONFIGURED, ctx.sofa_process_block, x[0], gains)   # channel 1 has none and is not dropped
        assert "no filter" in _raises(mi355fx.ERR_NOT_CONFIGURED, ctx.sofa_process_block, x[1], gains)
        ctx.sofa_set_drop(1, True)                    # the flags are still free: no block has run
        ctx.sofa_set_drop(1, False)
        for c in (ctx, never):
            c.sofa_set_filter(1, *flt[1])
        for b in range(2):
            S.same(ctx.sofa_process_block(x[b], gains), never.sofa_process_block(x[b], gains), b)
    finally:
        ctx.close()
        never.close()
