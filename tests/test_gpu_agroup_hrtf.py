"""hrtfrender members of an audio group (mi355_agroup_*_hrtf) against lone contexts, bit for bit.

The standing comparison is numpy.array_equal on the float32 output of a member against a lone Context given the same sphere
bytes and rate, FLAG_HRTF_METHOD = the member's method, and the same blocks, positions and gains; the faces and weights of the
last mesh lookup must be equal as well. No tolerance: the job-table kernels call the lone kernels' bodies.
The lone path itself is pinned by tests/golden/hrtf_lone_crc.json, written by tools/hrtf_lone_crc.py at the commit before the
bodies were shared."""
import json
import threading

import numpy as np
import pytest

import audio_state_cases as A
import hrtf_group_cases as H
import mi355fx

pytestmark = pytest.mark.gpu

UNIFORM = {"key": "uniform", "file_len": 256, "file_rate": 48000, "rate": 48000, "len": 256, "channels": 8, "steps": 8, "block": 512, "method": 0,
           "transform": 0}
SMALL = {"key": "small", "file_len": 256, "file_rate": 44100, "rate": 44100, "len": 256, "channels": 3, "steps": 4, "block": 128, "method": 0,
         "transform": 0}
SMALL_FFT = dict(SMALL, key="small_fft", file_len=400, len=400, channels=2, transform=1024, block=512)


def _join(g, synth, idx, m, sphere=None):
    """member idx of g loaded and set up as m; -> the lone context that is its yardstick"""
    sp = sphere if sphere is not None else H.sphere_bytes(synth, m)
    g.hrtf_load_sphere(idx, sp, m["rate"])
    g.hrtf_setup(idx, m["channels"], m["block"], m["steps"], m["method"])
    return H.lone_context(mi355fx, synth, m, sp)


def _same(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]), float(np.abs(got - want).max()))


def _interval(g, lone, streams, blk, who=None, frames=None):
    """one interval from one thread: every member of `who` submits block streams[m][blk[m]], then each waits; compared with its lone context"""
    who = list(range(len(lone))) if who is None else who
    tickets = {m: g.submit_hrtf(m, *streams[m][blk[m]]) for m in who}
    for m in who:
        n = g.wait(tickets[m])
        if frames is not None:
            assert n == frames[m]
    for m in who:
        want = lone[m].hrtf_process_block(*streams[m][blk[m]])
        _same(g.hrtf_output(m), want, (m, blk[m]))
        gf, gw = g.hrtf_last_lookup(m)
        lf, lw = lone[m].hrtf_last_lookup()
        assert np.array_equal(gf, lf) and np.array_equal(gw, lw), (m, blk[m])
        blk[m] += 1


def test_heterogeneous_set_equals_lone_contexts(mi355lib, synth):
    """nine members - both convolution forms, three transform sizes, 1 .. 64 channels, a resampled sphere - in every launch set"""
    ms = H.members()
    assert len(ms) == 9
    g = mi355fx.AudioGroup("hrtf", len(ms))
    lone = []
    try:
        for i, m in enumerate(ms):
            lone.append(_join(g, synth, i, m))
            length, fft_n, _ = g.hrtf_info(i)
            assert length == m["len"]
            # which form serves is asserted, not assumed: both forms and three transform sizes are in the set
            assert fft_n == A.hrtf_expected_transform(m["len"], m["block"], m["method"]) == m["transform"] == lone[i].hrtf_transform_size()
        assert sorted({m["transform"] for m in ms}) == [0, 1024, 2048, 4096]
        assert g.hrtf_info(0)[2] == 9   # nine different spheres
        n_blocks = 5
        streams = [H.stream(m, n_blocks) for m in ms]
        blk = [0] * len(ms)
        for _ in range(n_blocks):
            _interval(g, lone, streams, blk, frames=[m["steps"] * m["block"] for m in ms])
        assert g.stats() == (9 * n_blocks, n_blocks, 9)   # one launch set per interval, nine buffers in each
        # prepare + one launch per transform size present (1024, 2048, 4096) + one for the FIR rows + mix
        assert g.hrtf_launches() == 6 * n_blocks
    finally:
        for c in lone:
            c.close()
        g.close()


def test_uniform_set_shares_one_sphere_and_three_launches(mi355lib, synth):
    n = 32
    sp = H.sphere_bytes(synth, UNIFORM)
    g = mi355fx.AudioGroup("hrtf", n)
    lone = []
    try:
        for i in range(n):
            lone.append(_join(g, synth, i, UNIFORM, sp))
        assert all(g.hrtf_info(i) == (256, 0, 1) for i in range(n))   # identical bytes at one rate: ONE device copy
        n_blocks = 4
        streams = [H.stream(UNIFORM, n_blocks, seed=i + 1) for i in range(n)]
        blk = [0] * n
        for _ in range(n_blocks):
            _interval(g, lone, streams, blk)
        assert g.stats() == (n * n_blocks, n_blocks, n)
        assert g.hrtf_launches() == 3 * n_blocks
    finally:
        for c in lone:
            c.close()
        g.close()


def test_spheres_are_shared_by_content_and_rate(mi355lib, synth):
    a, b = H.sphere_bytes(synth, SMALL), H.sphere_bytes(synth, SMALL, seed_offset=1)
    assert a != b and len(a) == len(b)
    g = mi355fx.AudioGroup("hrtf", 4)
    try:
        g.hrtf_load_sphere(0, a, 44100)
        g.hrtf_load_sphere(1, b, 44100)
        assert g.hrtf_info(0)[2] == 2
        g.hrtf_load_sphere(2, a, 44100)
        assert g.hrtf_info(0)[2] == 2
        g.hrtf_load_sphere(3, a, 48000)      # the same bytes at another device rate are another sphere (resampled)
        assert g.hrtf_info(0)[2] == 3 and g.hrtf_info(3)[0] == round(256 * 48000 / 44100)
        g.hrtf_load_sphere(1, a, 44100)      # the last holder of b lets go of it
        assert g.hrtf_info(0)[2] == 2
    finally:
        g.close()


def test_member_that_skips_an_interval(mi355lib, synth):
    ms = [SMALL, SMALL_FFT, SMALL]
    g = mi355fx.AudioGroup("hrtf", 3)
    g.set_linger(3000)   # a few ms: nobody waits on the member that does not come for longer than that
    lone = []
    try:
        for i, m in enumerate(ms):
            lone.append(_join(g, synth, i, m))
        streams = [H.stream(m, 4, seed=10 + i) for i, m in enumerate(ms)]
        blk = [0, 0, 0]
        _interval(g, lone, streams, blk)
        _interval(g, lone, streams, blk, who=[0, 1])      # member 2 does not come: the set runs without it after the linger
        assert blk == [2, 2, 1]
        assert g.stats() == (5, 2, 3)
        _interval(g, lone, streams, blk)                  # member 2's next block is its lone context's next block
        _interval(g, lone, streams, blk, who=[2])
        assert blk == [3, 3, 3] and g.stats()[:2] == (9, 4)
    finally:
        for c in lone:
            c.close()
        g.close()


def test_reset_of_one_member_between_blocks(mi355lib, synth):
    ms = [SMALL, SMALL, SMALL_FFT]
    g = mi355fx.AudioGroup("hrtf", 3)
    lone = []
    try:
        for i, m in enumerate(ms):
            lone.append(_join(g, synth, i, m))
        never_reset = H.lone_context(mi355fx, synth, SMALL)
        streams = [H.stream(m, 4, seed=20 + i) for i, m in enumerate(ms)]
        blk = [0, 0, 0]
        for _ in range(2):
            never_reset.hrtf_process_block(*streams[1][blk[1]])
            _interval(g, lone, streams, blk)
        g.hrtf_reset(1)          # tails gone, previous direction kept: the first step still interpolates from it
        lone[1].hrtf_reset()
        kept = never_reset.hrtf_process_block(*streams[1][2])
        _interval(g, lone, streams, blk)     # member 1 equals the lone context reset at the same point, its neighbours ones that were not
        faces, uvw = never_reset.hrtf_last_lookup()
        gf, gw = g.hrtf_last_lookup(1)
        assert np.array_equal(gf, faces) and np.array_equal(gw, uvw)        # the previous direction survived the reset
        assert not np.array_equal(g.hrtf_output(1), kept)                    # and the tail did not
        _interval(g, lone, streams, blk)
        never_reset.close()
    finally:
        for c in lone:
            c.close()
        g.close()


def test_device_buffers_equal_host_buffers(mi355lib, synth):
    ms = [SMALL, SMALL_FFT]
    g = mi355fx.AudioGroup("hrtf", 2)
    lone = []
    ctx = mi355fx.Context(0)
    try:
        for i, m in enumerate(ms):
            lone.append(_join(g, synth, i, m))
        streams = [H.stream(m, 4, seed=30 + i) for i, m in enumerate(ms)]
        frames = [m["steps"] * m["block"] for m in ms]
        d_in = [ctx.alloc(frames[i] * ms[i]["channels"] * 4) for i in range(2)]
        d_out = [ctx.alloc(frames[i] * 8) for i in range(2)]
        for b in range(4):
            device = [b % 2 == 0, True]     # member 0 alternates between host and device buffers, member 1 stays on the device
            tickets = []
            for i in range(2):
                x, pos, gains = streams[i][b]
                if device[i]:
                    ctx.h2d(d_in[i], x)
                    ctx.synchronize()
                    tickets.append(g.submit_hrtf(i, d_in[i], pos, gains, out=d_out[i]))
                else:
                    tickets.append(g.submit_hrtf(i, x, pos, gains))
            for i in range(2):
                assert g.wait(tickets[i]) == frames[i]
                if device[i]:
                    got = np.zeros(frames[i] * 2, np.float32)
                    ctx.d2h(got, d_out[i])
                else:
                    got = g.hrtf_output(i)
                _same(got, lone[i].hrtf_process_block(*streams[i][b]), (i, b))
        for d in d_in + d_out:
            ctx.free(d)
    finally:
        ctx.close()
        for c in lone:
            c.close()
        g.close()


def _threads(synth, make_group, n=16, intervals=6):
    """n Python threads, one member each: every member equals its lone context"""
    ms = [[SMALL, SMALL_FFT, UNIFORM][i % 3] for i in range(n)]
    spheres = {m["key"]: H.sphere_bytes(synth, m) for m in ms}
    results, errors = {}, []
    barrier = threading.Barrier(n)

    def member(i):
        try:
            g, idx = make_group(i)
            m = ms[i]
            g.hrtf_load_sphere(idx, spheres[m["key"]], m["rate"])
            g.hrtf_setup(idx, m["channels"], m["block"], m["steps"], m["method"])
            barrier.wait(60)
            outs = []
            for blk in H.stream(m, intervals, seed=40 + i):
                n_frames = g.wait(g.submit_hrtf(idx, *blk))
                assert n_frames == m["steps"] * m["block"]
                outs.append(g.hrtf_output(idx).copy())
            results[i] = outs
            barrier.wait(60)
            if g.shared:
                g.close()
        except Exception as e:   # noqa: BLE001 - reported below
            errors.append((i, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=member, args=(i,)) for i in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errors, errors
    for i, m in enumerate(ms):
        ctx = H.lone_context(mi355fx, synth, m, spheres[m["key"]])
        for b, blk in enumerate(H.stream(m, intervals, seed=40 + i)):
            _same(results[i][b], ctx.hrtf_process_block(*blk), (i, b))
        ctx.close()


def test_sixteen_threads_one_member_each(mi355lib, synth):
    g = mi355fx.AudioGroup("hrtf", 16)
    g.set_linger(5000)
    try:
        _threads(synth, lambda i: (g, i))
        buffers, sets, largest = g.stats()
        assert buffers == 16 * 6 and sets >= 6 and largest <= 16
        assert g.hrtf_info(0)[2] == 3
    finally:
        g.close()


def test_shared_group_last_release_destroys_it(mi355lib, synth):
    handles = {}
    lock = threading.Lock()

    def make(i):
        with lock:
            h = mi355fx.AudioGroup("hrtf", 16, shared=True)
            h.set_linger(5000)
            handles[i] = (h.member, h.h)
        return h, h.member

    _threads(synth, make)
    assert sorted(m for m, _ in handles.values()) == list(range(16))   # one group served all sixteen
    assert len({h for _, h in handles.values()}) == 1
    # every member has released: the group is gone, and a fresh one is made for the next element of this configuration
    fresh = mi355fx.AudioGroup("hrtf", 16, shared=True)
    try:
        assert fresh.member == 0 and fresh.stats() == (0, 0, 0)
    finally:
        fresh.close()


def test_zero_direction_is_silence_before_any_hit_and_previous_taps_afterwards(mi355lib, synth):
    m = dict(SMALL, channels=1)
    g = mi355fx.AudioGroup("hrtf", 1)
    lone = []
    try:
        lone.append(_join(g, synth, 0, m))
        rng = np.random.default_rng(5)
        frames = m["steps"] * m["block"]
        zero, there = np.zeros((1, 3), np.float32), np.array([[0.3, 0.5, -0.8]], np.float32)
        gains = np.ones(1, np.float32)
        blocks = [(rng.uniform(-1, 1, (frames, 1)).astype(np.float32), p, gains) for p in (zero, there, zero, zero)]
        blk = [0]
        _interval(g, lone, [blocks], blk)
        assert not g.hrtf_output(0).any() and (g.hrtf_last_lookup(0)[0] == -1).all()    # no face hit yet: silence
        _interval(g, lone, [blocks], blk)
        assert g.hrtf_output(0).any()
        _interval(g, lone, [blocks], blk)
        _interval(g, lone, [blocks], blk)      # prev and new both zero: no hit in any step, the previous taps keep rendering
        assert (g.hrtf_last_lookup(0)[0] == -1).all() and g.hrtf_output(0).any()
    finally:
        for c in lone:
            c.close()
        g.close()


def test_errors_mirror_the_lone_path(mi355lib, synth, ctx):
    sp = H.sphere_bytes(synth, SMALL)
    g = mi355fx.AudioGroup("hrtf", 2)
    e = mi355fx.AudioGroup("echo", 2, ring_len=16)
    x = np.zeros((SMALL["steps"] * SMALL["block"], 3), np.float32)
    pos, gains = np.zeros((3, 3), np.float32), np.ones(3, np.float32)

    def status(fn, *a):
        with pytest.raises(mi355fx.Mi355Error) as ex:
            fn(*a)
        return ex.value.status

    try:
        assert status(g.hrtf_setup, 0, 3, 128, 4, 0) == mi355fx.ERR_NOT_CONFIGURED          # setup before a sphere
        g.hrtf_load_sphere(0, sp, 44100)
        g._hrtf_shape = {0: (3, x.shape[0], 4), 5: (3, x.shape[0], 4), -1: (3, x.shape[0], 4)}
        assert status(g.submit_hrtf, 0, x, pos, gains) == mi355fx.ERR_NOT_CONFIGURED      # submit before setup
        for channels in (0, 65, -1):
            assert status(g.hrtf_setup, 0, channels, 128, 4, 0) == mi355fx.ERR_INVALID_ARG
        assert status(g.hrtf_setup, 0, 3, 128, 4, 3) == mi355fx.ERR_INVALID_ARG              # no such method
        for member in (-1, 5):
            assert status(g.hrtf_load_sphere, member, sp, 44100) == mi355fx.ERR_INVALID_ARG
            assert status(g.hrtf_setup, member, 3, 128, 4, 0) == mi355fx.ERR_INVALID_ARG
            assert status(g.hrtf_reset, member) == mi355fx.ERR_INVALID_ARG
            assert status(g.submit_hrtf, member, x, pos, gains) == mi355fx.ERR_INVALID_ARG
            assert status(g.hrtf_info, member) == mi355fx.ERR_INVALID_ARG
        assert status(g.hrtf_load_sphere, 0, b"XXXX" + sp[4:], 44100) == mi355fx.ERR_INVALID_ARG
        assert status(e.hrtf_setup, 0, 3, 128, 4, 0) == mi355fx.ERR_INVALID_ARG              # another kind's group
        g.hrtf_setup(0, 3, 128, 4, 0)
        L = mi355lib
        t = np.zeros(1, np.uint64)
        import ctypes as C
        fp = C.POINTER(C.c_float)
        for args in ((None, x.ctypes.data, pos.ctypes.data_as(fp), gains.ctypes.data_as(fp)), (x.ctypes.data, None, pos.ctypes.data_as(fp), gains.ctypes.data_as(fp)),
                     (x.ctypes.data, x.ctypes.data, None, gains.ctypes.data_as(fp)), (x.ctypes.data, x.ctypes.data, pos.ctypes.data_as(fp), None)):
            assert L.mi355_agroup_submit_hrtf(g.h, 0, *args, 0, t.ctypes.data_as(C.POINTER(C.c_uint64))) == mi355fx.ERR_INVALID_ARG
        assert L.mi355_agroup_hrtf_load_sphere(g.h, 0, None, 0, 44100) == mi355fx.ERR_INVALID_ARG
        # the lone path refuses more than 64 channels as well (HrtfVecGain holds 64 channels' directions and gains)
        ctx.hrtf_load_sphere(sp, 44100)
        assert status(ctx.hrtf_setup, 65, 128, 4) == mi355fx.ERR_INVALID_ARG
        ctx.hrtf_setup(64, 128, 4)
    finally:
        e.close()
        g.close()


def test_lone_path_still_produces_the_parent_commits_bits(mi355lib, synth):
    """the guard for sharing the kernels' bodies between the lone and the job-table form: CRC-32s of the lone path's outputs taken
    at the parent commit (tools/hrtf_lone_crc.py) still hold"""
    with open(H.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert doc["blocks"] == H.GUARD_BLOCKS
    for m in H.members():
        assert H.lone_crcs(mi355fx, synth, m) == doc["shapes"][m["key"]], m["key"]


@pytest.mark.parametrize("m", H.extra_members(), ids=[m["key"] for m in H.extra_members()])
def test_lone_reset_and_device_entry_still_produce_the_parent_commits_bits(mi355lib, synth, m):
    """the fixture's "extra" section, recorded at the commit before audio_fft.hpp took over the two files' shared helpers: a reset after the first
    of GUARD_BLOCKS blocks, and the device entry point"""
    with open(H.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert doc["extra"]["blocks"] == H.GUARD_BLOCKS
    assert H.lone_extra_crcs(mi355fx, synth, m) == doc["extra"]["shapes"][m["key"]], m["key"]


def test_lone_context_set_up_again_equals_a_fresh_one(mi355lib, synth):
    first, second = SMALL, SMALL_FFT
    sp = {m["key"]: H.sphere_bytes(synth, m) for m in (first, second)}
    ctx = H.lone_context(mi355fx, synth, first, sp[first["key"]])
    fresh = H.lone_context(mi355fx, synth, second, sp[second["key"]])
    try:
        for blk in H.stream(first, 2, seed=50):
            ctx.hrtf_process_block(*blk)
        # the same bytes again on the same context (a group shares spheres by content: here with itself), then another sphere and geometry
        ctx.hrtf_load_sphere(sp[first["key"]], first["rate"])
        assert ctx.hrtf_sphere_info()[0] == first["len"]
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.hrtf_transform_size()                # a load takes the processors down: setup has to follow
        assert e.value.status == mi355fx.ERR_NOT_CONFIGURED
        ctx.hrtf_load_sphere(sp[second["key"]], second["rate"])
        ctx.hrtf_load_sphere(sp[second["key"]], second["rate"])
        ctx.hrtf_setup(second["channels"], second["block"], second["steps"])
        assert ctx.hrtf_transform_size() == fresh.hrtf_transform_size() == second["transform"]
        for b, blk in enumerate(H.stream(second, 3, seed=51)):
            got, want = ctx.hrtf_process_block(*blk), fresh.hrtf_process_block(*blk)
            assert got.any()
            _same(got, want, b)
        gf, gw = ctx.hrtf_last_lookup()
        ff, fw = fresh.hrtf_last_lookup()
        assert np.array_equal(gf, ff) and np.array_equal(gw, fw)
        ctx.hrtf_teardown()
        ctx.hrtf_teardown()                           # nothing left to trip over
        ctx.hrtf_reset()                              # (a reset without processors is accepted and does nothing, as ever)
    finally:
        ctx.close()
        ctx.close()
        fresh.close()
