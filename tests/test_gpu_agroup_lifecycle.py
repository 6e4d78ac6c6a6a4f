"""The audio groups' submit / run / wait protocol (csrc/agroup.hip), for all five element kinds: rsaudioecho, agingradio,
ebur128level, audioloudnorm, hrtfrender.

The other group tests walk the polite path: every member submits, then waits exactly once. Here a member waits twice, submits or
reconfigures before it has collected its result, waits for tickets that are not its outstanding one, or detaches around a result.
Every misuse must be refused with ERR_INVALID_ARG and move nothing: afterwards every sample and every piece of carried state the
bindings expose (echo_state, agingradio_state, the five loudness readings and both peaks, loudnorm's following frame, hrtfrender's
following block and last lookup) still equals a single-instance Context fed the same buffers in the same order, with `==`
(include/mi355fx.h: "bit for bit"); no tolerance is involved. S1 .. S5 run on one thread with linger 0 and are deterministic.

What each script does against the code before the life cycle was made explicit (one outstanding buffer per member, a ticket
collected once), from reading that code - NOT observed: no run of this file on a GPU, against either version of the library,
had been possible when it was written:
  S1 fails for every kind (nothing changed res_interval after a wait: the second wait answers OK and copies the slot out again);
  S2 fails for every kind, host and device members (run_interval cleared `have`: a second submit is accepted once the set has run);
  S3 fails for all five calls (agingradio_setup, ebur128_reset, hrtf_setup, hrtf_reset, hrtf_load_sphere pass the same check);
  S4 fails for every kind at one step only: waiting for the current interval's ticket value of a member that has not submitted
     is refused, but runs the launch set of the members that have on the way (stats() shows it); every other step passes;
  S5 passes for every kind; S6: see its docstring."""
import threading

import numpy as np
import pytest

import agingradio_restate as R
import hrtf_group_cases as H
import loudnorm_cases as LC
import mi355fx

pytestmark = pytest.mark.gpu

KINDS = ["echo", "agingradio", "ebur128", "loudnorm", "hrtf"]
N_M = 3
SENTINEL = -12345.5      # exact in f32 and f64; no kind produces it


def _refused(fn, *a, text=None, **kw):
    """the call raises Mi355Error with ERR_INVALID_ARG (and `text` in its message)"""
    with pytest.raises(mi355fx.Mi355Error) as e:
        fn(*a, **kw)
    assert e.value.status == mi355fx.ERR_INVALID_ARG, (e.value.status, str(e.value))
    if text is not None:
        assert text in str(e.value), str(e.value)


class Job:
    """one buffer of one member: `orig` is what the element was handed, `x` the array submitted (in place for echo and agingradio),
    `res` the caller's array the result arrives in (None: ebur128level has none, a device member's is read back)"""

    def __init__(self, member, orig, extra=()):
        self.member, self.orig, self.extra = member, orig, extra
        self.x, self.res, self.ticket, self.final = orig.copy(), None, None, False


class Adaptor:
    """a group of N_M members of one kind and the single-instance Contexts that are their yardstick"""
    in_place = False

    def __init__(self, synth=None, device_member=None):
        self.k = [0] * N_M            # buffers handed out per member
        self.device_member = device_member
        self.dev = mi355fx.Context(0) if device_member is not None else None
        self.dptr = {}
        self.singles, self.g = [], None
        try:
            self.open(synth)
            self.g.set_linger(0)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.g is not None:
            self.g.close()
        for p in self.dptr.values():
            self.dev.free(p)
        for c in self.singles + ([self.dev] if self.dev else []):
            c.close()

    def job(self, m):
        """the member's next buffer (a new Job; nothing is submitted yet)"""
        j = self.make(m, self.k[m])
        self.k[m] += 1
        return j

    def submit(self, j):
        j.ticket = self._submit(j)
        return j.ticket

    def wait(self, j):
        n = self.g.wait(j.ticket)
        j.frames = n
        return n

    def check(self, j):
        """feeds the buffer to the member's single instance (once per buffer, in order) and compares what the group delivered"""
        want = self.single(j)
        got = self.got(j)
        assert got.dtype == want.dtype and got.shape == want.shape, (self.name, j.member, got.shape, want.shape)
        assert (got == want).all(), (self.name, j.member, int(np.flatnonzero(got != want)[0]))

    def got(self, j):
        return j.res

    def spoil(self, j):
        """the caller's result array is overwritten with the sentinel; -> a function that asserts it is still untouched"""
        if j.res is None:
            return lambda: None
        j.res[...] = SENTINEL

        def untouched():
            assert (j.res == SENTINEL).all(), (self.name, j.member)
        return untouched

    def unmodified(self, j):
        """a buffer whose submit was refused still holds what the caller put there, and its output array nothing"""
        assert (j.x == j.orig).all()
        if not self.in_place and j.res is not None:
            assert not j.res.any()

    def check_state(self, members=range(N_M)):
        """every piece of carried state the bindings expose; for loudnorm and hrtfrender: the following frame / block"""
        for m in members:
            self.state_equal(m)

    def following(self, m):
        j = self.job(m)
        self.submit(j)
        self.wait(j)
        self.check(j)


class Echo(Adaptor):
    name, in_place = "echo", True
    RING = 4096
    PAR = [(1000, 0.5, 0.3), (0, 0.6, 0.0), (4096, 0.25, 0.9)]      # delay 0 reads the slot written a ring ago
    N = [300, 500, 257]
    DT = [np.float32, np.float64, np.float32]

    def open(self, synth):
        self.g = mi355fx.AudioGroup("echo", N_M, ring_len=self.RING)
        for _ in range(N_M):
            c = mi355fx.Context(0)
            self.singles.append(c)
            c.echo_setup(self.RING)

    def make(self, m, k):
        rng = np.random.default_rng(100 * m + k)
        return Job(m, rng.standard_normal(self.N[m]).astype(self.DT[m]))

    def _submit(self, j):
        m = j.member
        if m == self.device_member:
            if m not in self.dptr:
                self.dptr[m] = self.dev.alloc(j.x.nbytes)
            self.dev.h2d(self.dptr[m], j.x.view(np.uint8))
            self.dev.synchronize()
            return self.g.submit_echo(m, self.dptr[m], *self.PAR[m], n=j.x.size, is_f64=j.x.dtype == np.float64)
        j.res = j.x
        return self.g.submit_echo(m, j.x, *self.PAR[m])

    def got(self, j):
        if j.member == self.device_member:
            back = np.zeros_like(j.orig)
            self.dev.d2h(back.view(np.uint8), self.dptr[j.member])
            return back
        return j.res

    def single(self, j):
        return self.singles[j.member].echo_process(j.orig.copy(), *self.PAR[j.member])

    def state_equal(self, m):
        r1, p1 = self.g.echo_state(m, self.RING)
        r0, p0 = self.singles[m].echo_state(self.RING)
        assert p1 == p0 and (r1 == r0).all(), ("echo_state", m)


class Aging(Adaptor):
    name, in_place = "agingradio", True
    FRAMES = 100
    CH = [1, 2, 2]
    DT = [np.float32, np.float64, np.float32]
    S = dict(R.DEFAULTS, clicks_prob=0.01)

    def open(self, synth):
        self.g = mi355fx.AudioGroup("agingradio", N_M)
        self.ch = list(self.CH)
        for m in range(N_M):
            c = mi355fx.Context(0)
            self.singles.append(c)
            self.setup(m, self.CH[m])

    def setup(self, m, channels, seed=None):
        seed = 77 + m if seed is None else seed
        self.g.agingradio_setup(m, channels, 48000, 2000, seed)
        self.singles[m].agingradio_setup(channels, 48000, 2000, seed)
        self.ch[m] = channels

    def make(self, m, k):
        rng = np.random.default_rng(200 * m + k)
        return Job(m, rng.uniform(-1.2, 1.2, self.FRAMES * self.ch[m]).astype(self.DT[m]))

    def _submit(self, j):
        m = j.member
        if m == self.device_member:
            if m not in self.dptr:
                self.dptr[m] = self.dev.alloc(j.x.nbytes)
            self.dev.h2d(self.dptr[m], j.x.view(np.uint8))
            self.dev.synchronize()
            return self.g.submit_agingradio(m, self.dptr[m], self.S, frames=self.FRAMES, is_f64=j.x.dtype == np.float64)
        j.res = j.x
        return self.g.submit_agingradio(m, j.x, self.S, channels=self.ch[m])

    got = Echo.got

    def single(self, j):
        return self.singles[j.member].agingradio_process(j.orig.copy(), self.ch[j.member], self.S)

    def state_equal(self, m):
        y1, k1 = self.g.agingradio_state(m, self.ch[m])
        y0, k0 = self.singles[m].agingradio_state(self.ch[m])
        assert k1 == k0 and y1.tobytes() == y0.tobytes(), ("agingradio_state", m)


class Ebur128(Adaptor):
    name = "ebur128"
    RATE, CH, FRAMES = 48000, 2, 4800

    def open(self, synth):
        self.g = mi355fx.AudioGroup("ebur128", N_M, channels=self.CH, rate=self.RATE, mode=63)
        for _ in range(N_M):
            c = mi355fx.Context(0)
            self.singles.append(c)
            c.ebur128_setup(self.CH, self.RATE, 63)

    def make(self, m, k):
        rng = np.random.default_rng(300 * m + k)
        t = (k * self.FRAMES + np.arange(self.FRAMES)) / self.RATE
        x = np.stack([0.05 * (m + 1) * np.sin(2 * np.pi * (300.0 + 40 * m + 9 * c) * t) for c in range(self.CH)], 1) + 1e-3 * rng.standard_normal((self.FRAMES, self.CH))
        return Job(m, np.ascontiguousarray(x.astype(np.float32)).reshape(-1))

    def _submit(self, j):
        return self.g.submit_ebur128(j.member, j.x)

    def readings(self, m):
        g = self.g
        return [g.loudness(m, k) for k in range(5)] + [g.peak(m, c, tp) for tp in (False, True) for c in range(self.CH)]

    def single_readings(self, m):
        s = self.singles[m]
        return ([s.ebur128_loudness_momentary(), s.ebur128_loudness_shortterm(), s.ebur128_loudness_global(), s.ebur128_relative_threshold(),
                 s.ebur128_loudness_range()] + [s.ebur128_sample_peak(c) for c in range(self.CH)] + [s.ebur128_true_peak(c) for c in range(self.CH)])

    def check(self, j):
        assert j.frames == self.FRAMES
        self.singles[j.member].ebur128_add_frames(j.orig)
        self.state_equal(j.member)

    def state_equal(self, m):
        got, want = self.readings(m), self.single_readings(m)
        assert got == want, ("readings", m, got, want)


_LN = {}


def _ln_stream(m):
    """member m's stream, built once: its first frame, two 100 ms frames and a rest of 5000 + 7 m frames"""
    if m not in _LN:
        _LN[m] = LC.programme(LC.N0 + 2 * LC.F + 5000 + 7 * m, 1, 40 + m)
        _LN[m].setflags(write=False)
    return _LN[m]


class Loudnorm(Adaptor):
    name = "loudnorm"

    def open(self, synth):
        self.g = mi355fx.AudioGroup("loudnorm", N_M, channels=1)
        self.pos = [0] * N_M
        for _ in range(N_M):
            c = mi355fx.Context(0)
            self.singles.append(c)
            c.loudnorm_setup(1)

    def make(self, m, k):
        x = _ln_stream(m)
        assert k <= 3, "a stream is a first frame, two 100 ms frames and the rest"
        size = [LC.N0, LC.F, LC.F, len(x) - LC.N0 - 2 * LC.F][k]
        if k == 0:
            assert self.g.loudnorm_frame_size(m) == LC.N0      # its own first frame
        j = Job(m, x[self.pos[m]:self.pos[m] + size].copy())
        self.pos[m] += size
        j.final = k == 3
        j.res = np.zeros((31 * LC.F if j.final else LC.F, 1))
        return j

    def _submit(self, j):
        return self.g.submit_loudnorm(j.member, j.x, j.res, final_frame=j.final)

    def got(self, j):
        return j.res[:j.frames].reshape(-1)

    def single(self, j):
        c = self.singles[j.member]
        out = c.loudnorm_push(j.orig)
        if j.final:
            assert out.size == 0
            out = c.loudnorm_drain()
        return out

    def state_equal(self, m):
        self.following(m)


SMALL = {"key": "small", "file_len": 256, "file_rate": 44100, "rate": 44100, "len": 256, "channels": 3, "steps": 4, "block": 128, "method": 0,
         "transform": 0}      # the smallest block and interpolation-steps tests/test_gpu_agroup_hrtf.py uses; the FIR form
SMALL_FFT = dict(SMALL, key="small_fft", file_len=400, len=400, channels=2, transform=1024, block=512)      # the transform form


class Hrtf(Adaptor):
    name = "hrtf"
    MS = [SMALL, SMALL_FFT, SMALL]

    def open(self, synth):
        self.g = mi355fx.AudioGroup("hrtf", N_M)
        self.spheres = [H.sphere_bytes(synth, m) for m in self.MS]
        self.streams = [H.stream(m, 6, seed=50 + i) for i, m in enumerate(self.MS)]
        for i, m in enumerate(self.MS):
            self.g.hrtf_load_sphere(i, self.spheres[i], m["rate"])
            self.g.hrtf_setup(i, m["channels"], m["block"], m["steps"], m["method"])
            self.singles.append(H.lone_context(mi355fx, synth, m, self.spheres[i]))
            assert self.g.hrtf_info(i)[1] == m["transform"] == self.singles[i].hrtf_transform_size()

    def make(self, m, k):
        x, pos, gains = self.streams[m][k]
        return Job(m, x.reshape(-1), (pos, gains))

    def _submit(self, j):
        t = self.g.submit_hrtf(j.member, j.x, *j.extra)
        j.res = self.g.hrtf_output(j.member)
        return t

    def single(self, j):
        assert j.frames == self.MS[j.member]["steps"] * self.MS[j.member]["block"]
        return self.singles[j.member].hrtf_process_block(j.orig, *j.extra)

    def state_equal(self, m):
        self.following(m)
        gf, gw = self.g.hrtf_last_lookup(m)
        lf, lw = self.singles[m].hrtf_last_lookup()
        assert np.array_equal(gf, lf) and np.array_equal(gw, lw), ("last lookup", m)


ADAPTORS = {"echo": Echo, "agingradio": Aging, "ebur128": Ebur128, "loudnorm": Loudnorm, "hrtf": Hrtf}


@pytest.fixture()
def make(mi355lib, synth):
    made = []

    def _make(kind, **kw):
        made.append(ADAPTORS[kind](synth, **kw))
        return made[-1]
    yield _make
    for a in made:
        a.close()


# ---------------------------------------------------------------- S1: a ticket is collected once

@pytest.mark.parametrize("kind", KINDS)
def test_s1_a_ticket_is_collected_once(make, kind):
    a = make(kind)
    j = a.job(0)
    a.submit(j)
    a.wait(j)
    a.check(j)
    untouched = a.spoil(j)
    _refused(a.g.wait, j.ticket, text="waited for already")
    untouched()
    a.following(0)              # the refused wait moved no state: the member's next buffer is its single instance's next buffer
    a.check_state([0])
    if kind == "loudnorm":
        a.following(0)          # ... to the end of its stream: the final rest


# ---------------------------------------------------------------- S2: no second submit before the first result is collected

@pytest.mark.parametrize("kind,device_member", [(k, None) for k in KINDS] + [("echo", 2), ("agingradio", 2)])
def test_s2_no_second_submit_before_the_result_is_collected(make, kind, device_member):
    a = make(kind, device_member=device_member)
    first = [a.job(m) for m in range(N_M)]
    for j in first:
        a.submit(j)             # the third submit completes the set and runs it
    assert a.g.stats() == (3, 1, 3)
    a2 = a.job(0)
    held = first[0].res         # (what wait(first ticket) must fill: not replaced by the refused submit)
    _refused(a.submit, a2, text="has not been waited for")
    a.unmodified(a2)
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
    assert a.g.stats()[1] == 1  # the set has run; nobody has waited
    return jobs


def _collect(a, jobs):
    for j in jobs:
        a.wait(j)
        a.check(j)


def test_s3_agingradio_setup_is_refused_until_the_result_is_collected(make):
    """Member 0 has 1 channel and 100 frames of f32 outstanding: 400 bytes in its 4096-byte slot, the caller's array the first 100
    of 800 floats. A setup with 8 channels accepted in that window made wait size its copy by the NEW channel count: 3200 bytes,
    inside the slot and inside `big` - nothing outside memory this test owns was ever written."""
    a = make("agingradio")
    big = np.full(800, SENTINEL, np.float32)
    jobs = [a.job(m) for m in range(N_M)]
    x = big[:100]
    x[:] = jobs[0].orig
    jobs[0].x = x
    for j in jobs:
        a.submit(j)
    assert a.g.stats()[1] == 1
    _refused(a.g.agingradio_setup, 0, 8, 48000, 2000, 5, text="has not been waited for")
    _collect(a, jobs)
    assert (big[100:] == SENTINEL).all()
    a.check_state()
    a.setup(0, 8, seed=5)       # collected: the same call goes through
    a.following(0)
    a.check_state()


def test_s3_ebur128_reset_is_refused_until_the_result_is_collected(make):
    a = make("ebur128")
    _collect(a, _run_set(a))    # some history first: a reset that went through would show in every reading
    jobs = [a.job(m) for m in range(N_M)]
    for j in jobs:
        a.submit(j)
    _refused(a.g.ebur128_reset, 0, text="has not been waited for")
    _collect(a, jobs)
    a.g.ebur128_reset(0)
    a.singles[0].ebur128_reset()
    a.check_state()
    a.following(0)


@pytest.mark.parametrize("call", ["hrtf_setup", "hrtf_reset", "hrtf_load_sphere"])
def test_s3_hrtf_calls_are_refused_until_the_result_is_collected(make, synth, call):
    a = make("hrtf")
    m0 = a.MS[0]
    _collect(a, _run_set(a))    # tails and previous directions first: a reset or a setup that went through would show in the next block
    jobs = [a.job(m) for m in range(N_M)]
    for j in jobs:
        a.submit(j)
    args = {"hrtf_setup": (0, m0["channels"], m0["block"], m0["steps"], m0["method"]), "hrtf_reset": (0,),
            "hrtf_load_sphere": (0, a.spheres[0], m0["rate"])}[call]
    _refused(getattr(a.g, call), *args, text="has not been waited for")
    _collect(a, jobs)
    a.check_state()             # the following block: nothing of the member was reset
    getattr(a.g, call)(*args)   # collected: the same call goes through; the lone context does the same
    lone = a.singles[0]
    setup = (m0["channels"], m0["block"], m0["steps"])
    assert m0["method"] == 0    # (a lone context reads its method from FLAG_HRTF_METHOD, 0 unless set)
    if call == "hrtf_reset":
        lone.hrtf_reset()
    elif call == "hrtf_setup":
        lone.hrtf_setup(*setup)
    else:                       # the processors go with the sphere: set_caps builds them anew
        lone.hrtf_load_sphere(a.spheres[0], m0["rate"])
        a.g.hrtf_setup(0, *setup, m0["method"])
        lone.hrtf_setup(*setup)
    a.check_state([0])


# ---------------------------------------------------------------- S4: tickets that are not the member's outstanding one

@pytest.mark.parametrize("kind", KINDS)
def test_s4_tickets_that_are_not_outstanding(make, kind):
    a = make(kind)
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
    a.check_state()


# ---------------------------------------------------------------- S5: detach around a result (pins what the code does)

@pytest.mark.parametrize("kind", KINDS)
def test_s5_detach_before_the_set_has_run_drops_the_submission(make, kind):
    a = make(kind)
    j0, j1 = a.job(0), a.job(1)
    a.submit(j0)
    a.submit(j1)
    a.g.detach(1)
    assert a.g.stats() == (0, 0, 0)
    _refused(a.g.wait, j1.ticket, text="detached")
    a.unmodified(j1)
    j2 = a.job(2)
    a.submit(j2)                                    # completes the set of the members that are left
    assert a.g.stats() == (2, 1, 2)
    for j in (j0, j2):
        a.wait(j)
        a.check(j)
    a.check_state([0, 2])


@pytest.mark.parametrize("kind", KINDS)
def test_s5_detach_after_the_set_has_run_still_delivers_the_result(make, kind):
    a = make(kind)
    jobs = [a.job(m) for m in range(N_M)]
    for j in jobs:
        a.submit(j)
    assert a.g.stats() == (3, 1, 3)
    a.g.detach(1)
    for j in jobs:
        a.wait(j)
        a.check(j)
    a.check_state([0, 2])


# ---------------------------------------------------------------- S6: ebur128level's one sample format per launch set, under the copy window

S6_FRAMES_A = 2 * 131072      # stereo f32: 2 MiB, copied into its slot outside the group's lock (more than 64 KiB)
S6_TRIALS = 20


def test_s6_ebur128_formats_cannot_mix_under_the_copy_window(mi355lib):
    """Two meters, one launch set per trial (it runs when both have submitted). Thread A submits S6_FRAMES_A frames of f32 as
    member 0; thread B, released by an Event A sets immediately before its call, submits 4800 frames of s16 as member 1. Whatever
    the timing, per trial and per member: the submit was refused with ERR_INVALID_ARG and that meter did not move, or it was
    accepted and the meter's five readings and peaks equal a single meter fed the same buffer; and somebody was accepted.
    (While the set took its format from the last member that had submitted, B slipping in during A's copy made the whole set s16:
    member 0's floats were metered as 16-bit integers.)
    The size of A's buffer is NOT the measured one: the smallest size at which the code before the fix violates the invariant in
    3 of 5 runs, and twice that, were to be found on an MI355X, and no GPU run was possible when this was written. 2 MiB is an
    estimate (a copy of a few hundred microseconds against the tens of microseconds a released thread needs to arrive); the test
    was never seen to fail before the fix and stands as an invariant check."""
    rate, ch = 48000, 2
    g = mi355fx.AudioGroup("ebur128", 2, channels=ch, rate=rate, mode=63)
    singles = [mi355fx.Context(0) for _ in range(2)]
    for c in singles:
        c.ebur128_setup(ch, rate, 63)
    rng = np.random.default_rng(6)
    t = np.arange(S6_FRAMES_A) / rate
    xa = np.ascontiguousarray(np.stack([0.2 * np.sin(2 * np.pi * (440.0 + 30 * c) * t) for c in range(ch)], 1).astype(np.float32)).reshape(-1)
    xb = np.clip(np.rint(8000 * rng.standard_normal(4800 * ch)), -32768, 32767).astype(np.int16)
    bufs = [xa, xb]

    def readings(m):
        return [g.loudness(m, k) for k in range(5)] + [g.peak(m, c, tp) for tp in (False, True) for c in range(ch)]

    def single_readings(m):
        s = singles[m]
        return ([s.ebur128_loudness_momentary(), s.ebur128_loudness_shortterm(), s.ebur128_loudness_global(), s.ebur128_relative_threshold(),
                 s.ebur128_loudness_range()] + [s.ebur128_sample_peak(c) for c in range(ch)] + [s.ebur128_true_peak(c) for c in range(ch)])

    try:
        g.set_linger(0)
        for trial in range(S6_TRIALS):
            before = [readings(m) for m in range(2)]
            go = threading.Event()
            ticket, error = [None, None], [None, None]

            def element(m):
                try:
                    if m == 0:
                        go.set()
                    else:
                        go.wait(30)
                    ticket[m] = g.submit_ebur128(m, bufs[m])
                except mi355fx.Mi355Error as e:
                    error[m] = e

            ts = [threading.Thread(target=element, args=(m,)) for m in (1, 0)]
            for th in ts:
                th.start()
            for th in ts:
                th.join(60)
            assert not any(th.is_alive() for th in ts)
            assert ticket[0] is not None or ticket[1] is not None, (trial, error)
            for m in range(2):      # (a lone accepted member: linger 0, its wait runs the set of one)
                if ticket[m] is not None:
                    assert g.wait(ticket[m]) == bufs[m].size // ch
                    singles[m].ebur128_add_frames(bufs[m])
            for m in range(2):
                if ticket[m] is None:
                    assert error[m].status == mi355fx.ERR_INVALID_ARG and "one sample format" in str(error[m]), (trial, m, str(error[m]))
                    assert readings(m) == before[m], (trial, m)
                got, want = readings(m), single_readings(m)
                assert got == want, (trial, m, [ticket[k] is not None for k in range(2)], got, want)
    finally:
        g.close()
        for c in singles:
            c.close()
