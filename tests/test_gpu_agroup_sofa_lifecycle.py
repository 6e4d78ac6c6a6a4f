"""The audio groups' submit / run / wait protocol (csrc/agroup.hip) for kind `sofa`: the S1 .. S5 scripts of
tests/test_gpu_agroup_lifecycle.py (copied, not imported: that file stays as it is), plus one threaded run.

A member waits twice, submits or reconfigures (setup, set_filter, set_drop, reset) before it has collected its result, waits for
tickets that are not its outstanding one, or detaches around a result. Every misuse must be refused with ERR_INVALID_ARG and move
nothing: afterwards every block of every member still equals a lone Context fed the same blocks and filters in the same order, with
`==`. S1 .. S5 run on one thread with linger 0 and are deterministic."""
import threading

import numpy as np
import pytest

import audio_state_cases as A
import mi355fx
import sofa_group_cases as S

pytestmark = pytest.mark.gpu

N_M = 3
SENTINEL = -12345.5      # exact in f32; no block produces it
SHAPES = [(2, 50, 8, 64), (3, 64, 64, 64), (2, 50, 8, 64)]      # two partition lengths, one shared by two members
BLOCKS = 8


def _refused(fn, *a, text=None, **kw):
    """the call raises Mi355Error with ERR_INVALID_ARG (and `text` in its message)"""
    with pytest.raises(mi355fx.Mi355Error) as e:
        fn(*a, **kw)
    assert e.value.status == mi355fx.ERR_INVALID_ARG, (e.value.status, str(e.value))
    if text is not None:
        assert text in str(e.value), str(e.value)


class Job:
    """one block of one member: `orig` is what the element was handed, `x` the array submitted, `res` the array the result arrives in
    (None: a device member's is read back)"""

    def __init__(self, member, orig, gains):
        self.member, self.orig, self.gains = member, orig, gains
        self.x, self.res, self.ticket = orig.copy(), None, None


class Sofa:
    """a group of N_M sofalizer members and the lone Contexts that are their yardstick"""
    name = "sofa"

    def __init__(self, device_member=None):
        self.k = [0] * N_M            # blocks handed out per member
        self.device_member = device_member
        self.dev = mi355fx.Context(0) if device_member is not None else None
        self.dptr = {}
        self.singles, self.g = [], None
        try:
            self.g = mi355fx.AudioGroup("sofa", N_M)
            self.scheds = [S.schedule(s, seed=70 + i, blocks=BLOCKS) for i, s in enumerate(SHAPES)]
            for i, (s, sc) in enumerate(zip(SHAPES, self.scheds)):
                S.join(self.g, i, s, sc)
                self.singles.append(S.lone_context(mi355fx, s, sc))
            self.g.set_linger(0)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.g is not None:
            self.g.close()
        for pair in self.dptr.values():
            for p in pair:
                self.dev.free(p)
        for c in self.singles + ([self.dev] if self.dev else []):
            c.close()

    def job(self, m):
        """the member's next block (a new Job; nothing is submitted yet)"""
        x, gains, _ = self.scheds[m]["blocks"][self.k[m]]
        self.k[m] += 1
        return Job(m, x.reshape(-1), gains)

    def submit(self, j):
        m = j.member
        if m == self.device_member:
            if m not in self.dptr:
                self.dptr[m] = (self.dev.alloc(j.x.nbytes), self.dev.alloc(SHAPES[m][3] * 8))
            self.dev.h2d(self.dptr[m][0], j.x)
            self.dev.synchronize()
            j.ticket = self.g.submit_sofa(m, self.dptr[m][0], j.gains, out=self.dptr[m][1])
        else:
            j.ticket = self.g.submit_sofa(m, j.x, j.gains)
            j.res = self.g.sofa_output(m)
        return j.ticket

    def wait(self, j):
        j.frames = self.g.wait(j.ticket)
        return j.frames

    def got(self, j):
        if j.member == self.device_member:
            back = np.zeros(SHAPES[j.member][3] * 2, np.float32)
            self.dev.d2h(back, self.dptr[j.member][1])
            return back
        return j.res.reshape(-1)

    def check(self, j):
        """feeds the block to the member's lone context (once per block, in order) and compares what the group delivered"""
        assert j.frames == SHAPES[j.member][3]
        want = self.singles[j.member].sofa_process_block(j.orig, j.gains).reshape(-1)
        got = self.got(j)
        assert got.dtype == want.dtype and got.shape == want.shape, (j.member, got.shape, want.shape)
        assert (got == want).all(), (j.member, int(np.flatnonzero(got != want)[0]))

    def spoil(self, j):
        """the caller's result array is overwritten with the sentinel; -> a function that asserts it is still untouched"""
        if j.res is None:
            return lambda: None
        j.res[...] = SENTINEL

        def untouched():
            assert (j.res == SENTINEL).all(), j.member
        return untouched

    def unmodified(self, j):
        """a block whose submit was refused still holds what the caller put there"""
        assert (j.x == j.orig).all()

    def following(self, m):
        j = self.job(m)
        self.submit(j)
        self.wait(j)
        self.check(j)

    def check_state(self, members=range(N_M)):
        """what a member carries - delay lines, history, slot counter, filters - shows in its following block"""
        for m in members:
            self.following(m)


@pytest.fixture()
def make(mi355lib):
    made = []

    def _make(**kw):
        made.append(Sofa(**kw))
        return made[-1]
    yield _make
    for a in made:
        a.close()


# ---------------------------------------------------------------- S1: a ticket is collected once

def test_s1_a_ticket_is_collected_once(make):
    a = make()
    j = a.job(0)
    a.submit(j)
    a.wait(j)
    a.check(j)
    untouched = a.spoil(j)
    _refused(a.g.wait, j.ticket, text="waited for already")
    untouched()
    a.following(0)              # the refused wait moved no state: the member's next block is its lone context's next block
    a.check_state([0])


# ---------------------------------------------------------------- S2: no second submit before the first result is collected

@pytest.mark.parametrize("device_member", [None, 2], ids=["host", "device"])
def test_s2_no_second_submit_before_the_result_is_collected(make, device_member):
    a = make(device_member=device_member)
    first = [a.job(m) for m in range(N_M)]
    for j in first:
        a.submit(j)             # the third submit completes the set and runs it
    assert a.g.stats() == (3, 1, 3)
    a2 = a.job(0)
    held = first[0].res         # (what wait(first ticket) must fill: not replaced by the refused submit)
    _refused(a.submit, a2, text="has not been waited for")
    a.unmodified(a2)
    assert a.g.sofa_output(0) is held
    a.wait(first[0])
    assert first[0].res is held
    a.check(first[0])
    a.submit(a2)                # collected: the member is free again
    a.wait(a2)
    a.check(a2)
    for j in first[1:]:
        a.wait(j)
        a.check(j)
    a.check_state()


# ---------------------------------------------------------------- S3: no reconfiguration while a result is uncollected

def _run_set(a):
    jobs = [a.job(m) for m in range(N_M)]
    for j in jobs:
        a.submit(j)
    return jobs


def _collect(a, jobs):
    for j in jobs:
        a.wait(j)
        a.check(j)


@pytest.mark.parametrize("call", ["sofa_setup", "sofa_set_filter", "sofa_set_drop", "sofa_reset"])
def test_s3_sofa_calls_are_refused_until_the_result_is_collected(make, call):
    a = make()
    s0 = SHAPES[0]
    if call != "sofa_set_drop":
        _collect(a, _run_set(a))    # history first: a reset or a setup that went through would show in the next block
    sets = a.g.stats()[1]
    jobs = _run_set(a)
    assert a.g.stats()[1] == sets + 1   # the set has run; nobody has waited
    l2, r2 = A.sofa_filters(np.random.default_rng(9), 1, s0[1])[0]
    args = {"sofa_setup": (0,) + s0, "sofa_set_filter": (0, 1, l2, r2, 1, 0), "sofa_set_drop": (0, 1, True), "sofa_reset": (0,)}[call]
    pending = a.g.sofa_info(0)[2]
    _refused(getattr(a.g, call), *args, text="has not been waited for")
    assert a.g.sofa_info(0)[2] == pending == 0
    _collect(a, jobs)
    a.check_state()             # the following block: nothing of the member was reset, replaced or dropped
    lone = a.singles[0]
    if call == "sofa_set_drop":     # collected, but a block has run: refused for the lone path's reason now, by the lone path's status
        _refused(a.g.sofa_set_drop, *args, text="fixed once a block has been processed")
        _refused(lone.sofa_set_drop, 1, True, text="fixed once a block has been processed")
        a.check_state([0])
        return
    getattr(a.g, call)(*args)   # collected: the same call goes through; the lone context does the same
    if call == "sofa_reset":
        lone.sofa_reset()
    elif call == "sofa_set_filter":
        lone.sofa_set_filter(1, l2, r2, 1, 0)
    else:                       # set_caps builds the convolvers anew: no history, no filters
        lone.sofa_setup(*s0)
        for f in a.scheds[0]["filters"]:
            a.g.sofa_set_filter(0, *f)
            lone.sofa_set_filter(*f)
    a.check_state([0])


# ---------------------------------------------------------------- S4: tickets that are not the member's outstanding one

def test_s4_tickets_that_are_not_outstanding(make):
    a = make()
    g = a.g
    _refused(g.wait, 0)
    j0, j1 = a.job(0), a.job(1)
    a.submit(j0)
    a.submit(j1)                                    # interval 1: member 2 does not come
    assert j1.ticket == j0.ticket + 1
    _refused(g.wait, j0.ticket + 5 * N_M)           # a coming interval
    _refused(g.wait, j0.ticket + 2)                 # this interval's ticket value of member 2, which has not submitted
    assert g.stats() == (0, 0, 0)                   # ... and none of that ran the launch set of the two that have
    a.wait(j0)
    assert g.stats() == (2, 1, 2)
    a.check(j0)
    _refused(g.wait, j0.ticket + 2)                 # the same value once the interval has run without member 2
    a.wait(j1)
    a.check(j1)
    second = [a.job(m) for m in range(N_M)]         # interval 2
    for j in second:
        a.submit(j)
    for j in second:
        a.wait(j)
        a.check(j)
    untouched = [a.spoil(j) for j in (j0, second[0])]
    _refused(g.wait, j0.ticket)                     # member 0's ticket of interval 1 after it has completed interval 2
    _refused(g.wait, 0)
    _refused(g.wait, second[0].ticket + 7 * N_M)
    for u in untouched:
        u()
    assert g.stats() == (5, 2, 3)
    assert g.sofa_info(2)[2] == 0                   # member 2's filters waited for its first block, then ran with it
    a.check_state()


# ---------------------------------------------------------------- S5: detach around a result

def test_s5_detach_before_the_set_has_run_drops_the_submission(make):
    a = make()
    j0, j1 = a.job(0), a.job(1)
    a.submit(j0)
    a.submit(j1)
    a.g.detach(1)
    assert a.g.stats() == (0, 0, 0)
    _refused(a.g.wait, j1.ticket, text="detached")
    a.unmodified(j1)
    assert not j1.res.any()                         # its output array was never written
    j2 = a.job(2)
    a.submit(j2)                                    # completes the set of the members that are left
    assert a.g.stats() == (2, 1, 2)
    for j in (j0, j2):
        a.wait(j)
        a.check(j)
    a.check_state([0, 2])


def test_s5_detach_after_the_set_has_run_still_delivers_the_result(make):
    a = make()
    jobs = [a.job(m) for m in range(N_M)]
    for j in jobs:
        a.submit(j)
    assert a.g.stats() == (3, 1, 3)
    a.g.detach(1)
    for j in jobs:
        a.wait(j)
        a.check(j)
    a.check_state([0, 2])


# ---------------------------------------------------------------- threads: one member each

def test_eight_threads_one_member_each(mi355lib):
    n, intervals = 8, 6
    shapes = [[(2, 50, 8, 64), (3, 64, 64, 64), (2, 128, 64, 256)][i % 3] for i in range(n)]
    scheds = [S.schedule(s, seed=80 + i, blocks=intervals) for i, s in enumerate(shapes)]
    g = mi355fx.AudioGroup("sofa", n)
    g.set_linger(5000)
    results, errors = {}, []
    barrier = threading.Barrier(n)

    def member(i):
        try:
            S.join(g, i, shapes[i], scheds[i])
            barrier.wait(60)
            outs = []
            for (x, gains, changes) in scheds[i]["blocks"]:
                for f in changes:
                    g.sofa_set_filter(i, *f)
                assert g.wait(g.submit_sofa(i, x, gains)) == shapes[i][3]
                outs.append(g.sofa_output(i).copy())
            results[i] = outs
        except Exception as e:   # noqa: BLE001 - reported below
            errors.append((i, repr(e)))
            barrier.abort()

    try:
        ts = [threading.Thread(target=member, args=(i,)) for i in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not errors, errors
        assert not any(t.is_alive() for t in ts)
        buffers, sets, largest = g.stats()
        assert buffers == n * intervals and sets >= intervals and largest <= n
        for i in range(n):
            want = S.lone_outputs(mi355fx, shapes[i], scheds[i])
            for b in range(intervals):
                assert np.array_equal(results[i][b], want[b]), (i, b)
    finally:
        g.close()
