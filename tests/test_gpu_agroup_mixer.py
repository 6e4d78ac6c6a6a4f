"""Mixers as members of an audio group (csrc/agroup.hip, kind `mixer`): a member is one mixer - one room of a bridge server - and
ONE kernel launch serves every member that has submitted. Per member the result is that of a lone Context fed the same call, bit for
bit (and, through it, the restatement's); the submit / wait life cycle is the one tests/test_gpu_agroup_lifecycle.py pins for the
other kinds."""
import threading

import numpy as np
import pytest

import minus1mixer_cases as M
import minus1mixer_restate as R
import mi355fx

pytestmark = pytest.mark.gpu

F32, S16 = R.F32, R.S16
T = mi355fx.MIXER_FRAME_TILE
SIZES = [3, 1, 64, 5, 65, 2, 63, 8]                    # participants per member, cycled (member 1: a lone participant)
FRAMES = [480, T + 1, 0, 7, 2 * T + 3, T, 1, T - 1]    # frames per member, cycled (member 2: no frame at all)


def _refused(fn, *a, text=None, **kw):
    with pytest.raises(mi355fx.Mi355Error) as e:
        fn(*a, **kw)
    assert e.value.status == mi355fx.ERR_INVALID_ARG, (e.value.status, str(e.value))
    if text is not None:
        assert text in str(e.value), str(e.value)


def member_case(m, interval=0):
    """member m's interval: minus-1 rooms of different sizes and frame counts; every fifth member a general matrix"""
    n, frames = SIZES[m % len(SIZES)], FRAMES[(m + m // len(FRAMES)) % len(FRAMES)]
    seed = 5000 + 97 * m + interval
    if m % 5 == 4:
        return M.random_general(seed, n, n + 3, frames)
    return M.random_minus1(seed, n, frames)


def lone(ctx, case):
    ctx.mixer_setup(case.contrib)
    bufs = case.buffers()
    ctx.mixer_process(*case.call(bufs), case.frames)
    return bufs


def submit(g, m, case, bufs=None):
    bufs = case.buffers() if bufs is None else bufs
    return g.submit_mixer(m, *case.call(bufs), case.frames), bufs


def assert_equal_to_lone(ctx, bufs, case):
    for got, want in zip(bufs, lone(ctx, case)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), case.name
    M.assert_same(bufs, case)


@pytest.fixture()
def group(mi355lib):
    made = []

    def _make(n, **kw):
        made.append(mi355fx.AudioGroup("mixer", n, **kw))
        return made[-1]
    yield _make
    for g in made:
        g.close()


# ---------------------------------------------------------------- parity with lone contexts

@pytest.mark.parametrize("n_members", [1, 2, 32])
def test_members_equal_lone_contexts(ctx, group, n_members):
    g = group(n_members)
    g.set_linger(0)
    cases = [member_case(m) for m in range(n_members)]
    if n_members == 32:
        cases[31] = M.random_minus1(31, 256, T + 1)      # a full room among the small ones
    for m, c in enumerate(cases):
        g.mixer_setup(m, c.contrib)
    pending = [submit(g, m, c) for m, c in enumerate(cases)]
    assert g.mixer_launches() == (1 if any(c.frames for c in cases) else 0) and g.stats() == (n_members, 1, n_members)
    for (t, bufs), c in zip(pending, cases):
        assert g.wait(t) == c.frames
        assert_equal_to_lone(ctx, bufs, c)


def test_device_member_beside_host_members(ctx, group):
    g = group(3)
    g.set_linger(0)
    cases = [member_case(m) for m in (0, 3, 4)]
    for m, c in enumerate(cases):
        g.mixer_setup(m, c.contrib)
    c = cases[1]
    held, segs, outs, bufs1 = [], [], [], c.buffers()
    try:
        for inp, data, off in c.segments:
            p = ctx.alloc(data.nbytes + 16)
            held.append(p)
            ctx.h2d(p, data)
            segs.append((inp, (p, R.fmt_of(data), data.size), off))
        for b, (fmt, off, nch) in zip(bufs1, c.outputs):
            p = ctx.alloc(b.nbytes + 16)
            held.append(p)
            outs.append(((p, fmt), off, nch))
        ctx.synchronize()
        t0, b0 = submit(g, 0, cases[0])
        t1 = g.submit_mixer(1, segs, outs, c.frames, device_data=True)
        t2, b2 = submit(g, 2, cases[2])
        for t in (t0, t1, t2):
            g.wait(t)
        for b, (pf, _, _) in zip(bufs1, outs):
            ctx.d2h(b, pf[0])
    finally:
        for p in held:
            ctx.free(p)
    for bufs, case in ((b0, cases[0]), (bufs1, c), (b2, cases[2])):
        assert_equal_to_lone(ctx, bufs, case)


# ---------------------------------------------------------------- launch counts

def test_one_launch_per_full_interval(ctx, group):
    n = 4
    g = group(n)
    g.set_linger(0)
    for interval in range(3):
        before = g.mixer_launches()
        cases = [member_case(m, interval) for m in range(n)]
        for m, c in enumerate(cases):
            g.mixer_setup(m, c.contrib)
        pending = [submit(g, m, c) for m, c in enumerate(cases)]
        assert g.mixer_launches() == before + 1
        for (t, bufs), c in zip(pending, cases):
            g.wait(t)
            M.assert_same(bufs, c)
    assert g.stats() == (3 * n, 3, n)


def test_a_missing_member_costs_nothing_and_catches_up(ctx, group):
    n = 3
    g = group(n)
    g.set_linger(0)
    first = [member_case(m, 10) for m in (0, 3, 4)]  # (every one of them has frames: a set without a frame launches nothing)
    for m, c in enumerate(first):
        g.mixer_setup(m, c.contrib)
    t0, b0 = submit(g, 0, first[0])
    t1, b1 = submit(g, 1, first[1])
    assert g.mixer_launches() == 0                  # member 2 has not come
    g.wait(t0)                                      # linger 0: the two that are there run
    assert g.mixer_launches() == 1 and g.stats() == (2, 1, 2)
    g.wait(t1)
    assert_equal_to_lone(ctx, b0, first[0])
    assert_equal_to_lone(ctx, b1, first[1])
    t2, b2 = submit(g, 2, first[2])                 # the late member's interval: correct, in the next launch set
    g.wait(t2)
    assert g.mixer_launches() == 2
    assert_equal_to_lone(ctx, b2, first[2])


# ---------------------------------------------------------------- life cycle

def _three(group):
    g = group(3)
    g.set_linger(0)
    cases = [member_case(m) for m in (0, 3, 4)]
    for m, c in enumerate(cases):
        g.mixer_setup(m, c.contrib)
    return g, cases


def test_second_submit_and_setup_are_refused_while_one_is_outstanding(ctx, group):
    g, cases = _three(group)
    t0, b0 = submit(g, 0, cases[0])
    extra = cases[0].buffers()
    _refused(submit, g, 0, cases[0], extra, text="has not been waited for")          # submitted, not run
    _refused(g.mixer_setup, 0, R.minus1(7), text="has not been waited for")
    _refused(g.mixer_setup_minus1, 0, 7, text="has not been waited for")
    assert g.mixer_launches() == 0 and g.stats() == (0, 0, 0) and M.untouched(b0) and M.untouched(extra)
    pending = [(t0, b0)] + [submit(g, m, cases[m]) for m in (1, 2)]
    assert g.mixer_launches() == 1
    _refused(submit, g, 0, cases[0], extra, text="has not been waited for")          # run, not collected
    _refused(g.mixer_setup_minus1, 0, 7, text="has not been waited for")
    assert g.mixer_launches() == 1 and M.untouched(b0) and M.untouched(extra)
    for (t, bufs), c in zip(pending, cases):
        g.wait(t)
        assert_equal_to_lone(ctx, bufs, c)          # the refused setup changed nothing: the matrix is still the member's
    assert M.untouched(extra)


def test_tickets_are_collected_once_and_only_by_their_member(ctx, group):
    g, cases = _three(group)
    _refused(g.wait, 0)
    t0, b0 = submit(g, 0, cases[0])
    t1, b1 = submit(g, 1, cases[1])
    _refused(g.wait, t0 + 5 * 3)                    # a coming interval
    _refused(g.wait, t0 + 2)                        # this interval's ticket of member 2, which has not submitted
    assert g.mixer_launches() == 0 and M.untouched(b0) and M.untouched(b1)
    g.wait(t0)
    g.wait(t1)
    assert g.mixer_launches() == 1
    keep = [b.copy() for b in b0]
    for b in b0:
        b[...] = M.SENTINEL_S16 if b.dtype == np.int16 else M.SENTINEL_F32
    _refused(g.wait, t0, text="waited for already")
    _refused(g.wait, t0 + 2)
    assert g.mixer_launches() == 1 and M.untouched(b0)
    for b, k in zip(b0, keep):
        b[...] = k
    assert_equal_to_lone(ctx, b0, cases[0])
    assert_equal_to_lone(ctx, b1, cases[1])


def test_detach_before_the_set_runs_drops_the_buffer(ctx, group):
    g, cases = _three(group)
    t0, b0 = submit(g, 0, cases[0])
    t1, b1 = submit(g, 1, cases[1])
    g.detach(1)
    assert g.mixer_launches() == 0
    _refused(g.wait, t1, text="detached")
    assert M.untouched(b1)
    t2, b2 = submit(g, 2, cases[2])                 # completes the set of the members that are left
    assert g.mixer_launches() == 1 and g.stats() == (2, 1, 2)
    g.wait(t0)
    g.wait(t2)
    assert_equal_to_lone(ctx, b0, cases[0])
    assert_equal_to_lone(ctx, b2, cases[2])
    assert M.untouched(b1)


def test_a_setup_between_intervals_takes_effect(ctx, group):
    g = group(2)
    g.set_linger(0)
    for k, n in enumerate((3, 5, 2)):
        cases = [M.random_minus1(600 + k, n, T + 1), M.random_minus1(700 + k, 4, 7)]
        g.mixer_setup_minus1(0, n)
        if k == 0:
            g.mixer_setup_minus1(1, 4)
        pending = [submit(g, m, c) for m, c in enumerate(cases)]
        for (t, bufs), c in zip(pending, cases):
            g.wait(t)
            assert_equal_to_lone(ctx, bufs, c)


def test_submit_before_setup_and_bad_arguments_are_refused(group):
    g = group(2)
    g.set_linger(0)
    case = M.random_minus1(1, 3, 8)
    bufs = case.buffers()
    with pytest.raises(mi355fx.Mi355Error) as e:
        submit(g, 0, case, bufs)
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED
    g.mixer_setup_minus1(0, 2)                      # the case names input 2: one too many for this room
    _refused(submit, g, 0, case, bufs)
    with pytest.raises(mi355fx.Mi355Error) as e:
        g.mixer_setup_minus1(0, 257)
    assert e.value.status == mi355fx.ERR_UNSUPPORTED
    assert M.untouched(bufs) and g.mixer_launches() == 0 and g.stats() == (0, 0, 0)


# ---------------------------------------------------------------- threads and shared groups

def test_eight_threads_one_member_each(ctx, mi355lib):
    n, intervals = 8, 20
    g = mi355fx.AudioGroup("mixer", n)
    g.set_linger(5000)
    cases = [[member_case(m, 100 + k) for k in range(intervals)] for m in range(n)]
    results, errors = {}, []
    barrier = threading.Barrier(n)

    def member(m):
        try:
            barrier.wait(60)
            outs = []
            for c in cases[m]:
                g.mixer_setup(m, c.contrib)          # (a general member's matrix changes from interval to interval)
                t, bufs = submit(g, m, c)
                assert g.wait(t) == c.frames
                outs.append(bufs)
            results[m] = outs
        except Exception as e:   # noqa: BLE001 - reported below
            errors.append((m, repr(e)))
            barrier.abort()

    try:
        ts = [threading.Thread(target=member, args=(m,)) for m in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not errors, errors
        assert not any(t.is_alive() for t in ts)
        buffers, sets, largest = g.stats()
        assert buffers == n * intervals and sets >= intervals and largest <= n
        for m in range(n):
            for k, c in enumerate(cases[m]):
                M.assert_same(results[m][k], c)
        for m in (0, 4):                             # and against lone contexts, for a minus-1 and a general member
            assert_equal_to_lone(ctx, results[m][intervals - 1], cases[m][intervals - 1])
    finally:
        g.close()


def test_shared_groups_hand_out_members_then_start_a_new_group(mi355lib):
    n = 3
    held = [mi355fx.AudioGroup("mixer", n, shared=True) for _ in range(n + 1)]
    try:
        assert [a.member for a in held] == [0, 1, 2, 0]
        assert held[0].h == held[1].h == held[2].h and held[3].h != held[0].h
        case = M.random_minus1(9, 3, T + 1)
        a = held[3]                                  # alone in its group so far: its set is complete with its own submit
        a.set_linger(0)
        a.mixer_setup_minus1(a.member, 3)
        t, bufs = submit(a, a.member, case)
        a.wait(t)
        M.assert_same(bufs, case)
    finally:
        for a in held:
            a.close()
