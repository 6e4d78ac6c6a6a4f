"""GPU parity tests for audioloudnorm through the C ABI against the CPU oracle.

The gain history is kept on the host; the per-sample loops and the limiter with its peak search run as kernels, for a
single context (a batch of one stream behind loudnorm_push / _drain) as for a batch. Everything in-tree is f64 and
unfused, so the samples must be BIT-IDENTICAL to the oracle as long as the two loudness meters agree; the meters (device vs oracle) agree to ~1e-9 LU (tests/test_gpu_ebur128.py), which
enters the samples only through pow(10, x/20) of the gain history: tolerance 1e-9 relative, and bit-exact is asserted
where no meter-dependent gain is involved (linear path excluded: offset depends on the global loudness).
What a single context gives is, in addition, what it gave when it still ran a host-driven limiter of its own: the hashes of
tests/golden/loudnorm_lone_parent.json (tests/loudnorm_streams.py)."""
import numpy as np
import pytest

import loudnorm_streams as LS
from loudnorm_streams import RATE, tone as _tone

pytestmark = pytest.mark.gpu


def _both(ctx, oracle, name, x=None):
    """stream `name` of tests/loudnorm_streams.py through the context and the oracle -> (input, context's output, oracle's output);
    the context's output is asserted to be the one recorded in tests/golden/loudnorm_lone_parent.json on the way"""
    st = LS.get(name)
    if x is None:
        x = st.make()
    ch = x.shape[1]
    ln = oracle.LoudNorm(ch, **st.kw)
    ctx.loudnorm_setup(ch, **st.kw)
    got, exp = [], []
    for part in st.parts(x):
        g, e = ctx.loudnorm_push(part), ln.push(part)
        assert g.size == e.size
        got.append(g); exp.append(e)
    g, e = ctx.loudnorm_drain(), ln.drain()
    assert (g is None) == (e is None)
    if g is not None:
        assert g.size == e.size
        got.append(g); exp.append(e)
    got = np.concatenate(got)
    LS.check(name, x, got)
    return x, got, np.concatenate(exp)


def _close(got, exp):
    scale = max(1e-12, float(np.abs(exp).max()))
    return float(np.abs(got - exp).max()) / scale


@pytest.mark.parametrize("ch", [1, 2, 6])
def test_limiter_heavy_stream_matches_oracle(ctx, oracle, ch):
    """Bursts far above the ceiling in every limiter situation: isolated, rising series (attack restarts), falling
    series (sustain), a burst inside the release window, one in the first 10 ms, one near the very end."""
    x, got, exp = _both(ctx, oracle, "limiter_heavy/%dch" % ch)
    assert got.size == x.size
    assert np.abs(got).max() <= 10 ** (-2.0 / 20)
    assert _close(got, exp) <= 1e-9


def test_quiet_then_loud_gain_tracking(ctx, oracle):
    """Silence (below -70 LUFS: above_threshold stays false), then programme material: exercises the delta history,
    the gaussian smoothing and the 1.0058 creep (imp.rs:560-575)."""
    x, got, exp = _both(ctx, oracle, "quiet_then_loud")
    assert _close(got, exp) <= 1e-9


def test_short_stream_linear_path_and_empty(ctx, oracle):
    x, got, exp = _both(ctx, oracle, "short_stream")
    assert got.size == x.size and _close(got, exp) <= 1e-9
    ctx.loudnorm_setup(2)
    assert ctx.loudnorm_drain() is None   # FlowError::Eos


def test_settings_and_exactly_three_seconds(ctx, oracle):
    x, got, exp = _both(ctx, oracle, "exactly_three_seconds")
    assert got.size == x.size
    assert np.abs(got).max() <= 10 ** (-1.0 / 20)
    assert _close(got, exp) <= 1e-9


def test_not_negotiated(ctx):
    import mi355fx
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx._ln_channels = 1
        ctx.loudnorm_push(np.zeros(10))
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED


# ------------------------------------------------------------------ batches of streams (round 3)

def _run_batch(ctx, streams, ch, **kw):
    """feeds the batch the way drain_full_frames does: whole frames, then the rest at drain"""
    S = len(streams)
    ctx.loudnorm_setup_batch(S, ch, **kw)
    n = len(streams[0])
    outs, pos = [], 0
    while True:
        need = ctx.loudnorm_batch_frame_size()
        if n - pos < need:
            break
        outs.append(ctx.loudnorm_process_batch(np.stack([s[pos:pos + need].reshape(-1) for s in streams])))
        pos += need
    outs.append(ctx.loudnorm_process_batch(np.stack([s[pos:].reshape(-1) for s in streams]), final=True))
    ctx.loudnorm_teardown()
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("ch,seconds", [(2, 5.23), (1, 3.0), (6, 3.71)])
def test_batch_equals_separate_streams_and_oracle(ctx, oracle, ch, seconds):
    """n streams in lock step, the limiter's state machine on the device: every stream's samples equal those of a separate
    single-stream context BIT FOR BIT (same expressions, same meters) and the oracle's within the meters' 1e-9."""
    import mi355fx
    S = 5
    streams = LS.batch_streams(ch, seconds)
    assert len(streams) == S
    got = _run_batch(ctx, streams, ch)
    assert got.shape == (S, int(seconds * RATE) * ch)
    for s in range(S):
        with mi355fx.Context(0) as c1:
            _, single, exp = _both(c1, oracle, "batch_single/%dch/%d" % (ch, s), streams[s])
        assert (got[s] == single).all(), (s, int((got[s] != single).sum()))
        assert _close(got[s], exp) <= 1e-9
        assert np.abs(got[s]).max() <= 10 ** (-2.0 / 20)


def test_batch_short_streams_take_the_linear_path(ctx, oracle):
    """less than 3 s in all: process_first_frame_is_last (imp.rs:334-366), a per-stream linear gain"""
    streams = [_tone(1.3, 2, amp=0.05 * (s + 1)) for s in range(3)]
    got = _run_batch(ctx, streams, 2, loudness_target=-20.0)
    for s in range(3):
        ln = oracle.LoudNorm(2, loudness_target=-20.0)
        assert ln.push(streams[s]).size == 0
        assert _close(got[s], ln.drain()) <= 1e-9


def test_batch_argument_checks(ctx):
    import mi355fx
    ctx.loudnorm_setup_batch(2, 2)
    assert ctx.loudnorm_batch_frame_size() == 3 * RATE
    with pytest.raises(mi355fx.Mi355Error):
        ctx.loudnorm_process_batch(np.zeros((2, 100 * 2)))   # not a whole frame
    ctx.loudnorm_teardown()
    assert ctx.loudnorm_batch_frame_size() == 0


def test_single_state_and_batch_share_a_context(ctx):
    """One context holds a single-stream state and a batch of two at once, calls interleaved frame by frame: each gives, bit for
    bit, what a fresh context that ran only it gives. Mono, 3 s + 2.5 frames (3 s is the smallest first frame there is), one
    burst above the ceiling in the second inner frame of every stream."""
    import mi355fx
    F, N0 = 19200, 3 * RATE
    n = N0 + 2 * F + F // 2
    xs = []
    for k in range(3):
        x = _tone((n + 1) / RATE, 1, amp=0.02 * (k + 1), f=330.0 + 50 * k)[:n]
        i = N0 + F + 3000 + 2500 * k
        x[i:i + 40 + 10 * k] *= 60.0
        xs.append(x)
    lone, rows = xs[0], xs[1:]
    cuts = [0, N0, N0 + F, N0 + 2 * F]

    def run(c, with_lone, with_batch):
        out_l, out_b = [], []
        if with_lone:
            c.loudnorm_setup(1)
        if with_batch:
            c.loudnorm_setup_batch(2, 1)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if with_lone:
                out_l.append(c.loudnorm_push(lone[a:b]))
            if with_batch:
                assert c.loudnorm_batch_frame_size() == b - a
                out_b.append(c.loudnorm_process_batch(np.stack([r[a:b].reshape(-1) for r in rows])))
        if with_lone:
            out_l.append(c.loudnorm_push(lone[cuts[-1]:]))
        if with_batch:
            out_b.append(c.loudnorm_process_batch(np.stack([r[cuts[-1]:].reshape(-1) for r in rows]), final=True))
        if with_lone:
            out_l.append(c.loudnorm_drain())
        c.loudnorm_teardown()
        return (np.concatenate(out_l) if with_lone else None), (np.concatenate(out_b, axis=1) if with_batch else None)

    both_l, both_b = run(ctx, True, True)
    with mi355fx.Context(0) as c1:
        only_l, _ = run(c1, True, False)
    with mi355fx.Context(0) as c2:
        _, only_b = run(c2, False, True)
    assert both_l.size == n and both_b.shape == (2, n)
    ceiling = 10 ** (-2.0 / 20)
    assert 0.5 * ceiling < np.abs(both_l[N0 + F:N0 + 2 * F]).max() <= ceiling   # the burst came out, held at the ceiling
    assert (both_l == only_l).all(), int((both_l != only_l).sum())
    assert (both_b == only_b).all(), int((both_b != only_b).sum())


# ------------------------------------------------------------------ the case table (tests/loudnorm_cases.py)
#
# Every case is pinned on the CPU first (tests/test_loudnorm_cpu.py): the oracle equals an independent restatement of imp.rs bit
# for bit there, and the limiter branches the case reaches are known by name. Here lnb_limiter_kernel runs the same streams, as the
# one stream of a single context and as one of a batch of four. The "grid" cases keep every delta at exactly 1.0 (input below
# -70 LUFS, the gain is the +60 dB offset: no meter reading enters a sample), so they are asserted BIT-IDENTICAL to the oracle; the
# programme cases at the meters' 1e-9.

import loudnorm_cases as LC


def _case_single(oracle, case):
    """(single-stream context output, oracle output) of a case"""
    import mi355fx
    ln = oracle.LoudNorm(case.channels, **case.kw)
    got, exp = [], []
    with mi355fx.Context(0) as c1:
        c1.loudnorm_setup(case.channels, **case.kw)
        for part in case.chunks():
            g, e = c1.loudnorm_push(part), ln.push(part)
            assert g.size == e.size
            got.append(g); exp.append(e)
        g, e = c1.loudnorm_drain(), ln.drain()
        assert g is not None and e is not None and g.size == e.size
        got.append(g); exp.append(e)
    got = np.concatenate(got)
    LS.check("case/" + case.name, case.x, got)
    return got, np.concatenate(exp)


def _fillers(case):
    """streams of the case's length whose limiter is somewhere else at every moment: the case itself 5000 frames late, programme
    with bursts at other places, and one that never leaves Out"""
    n, ch = case.x.shape
    late = np.roll(case.x, 5000, axis=0)
    rng = np.random.default_rng(len(case.name))
    prog = _tone((n + 1) / RATE, ch, amp=0.03, f=517.0)[:n]
    for _ in range(8):
        i = int(rng.integers(0, n - 4000))
        prog[i:i + int(rng.integers(10, 3000))] *= rng.uniform(20.0, 90.0)
    if case.kw.get("offset"):
        prog *= 10 ** (-case.kw["offset"] / 20.0)
    return [late, prog, _tone((n + 1) / RATE, ch, amp=1e-9)[:n]]


@pytest.mark.parametrize("name", LC.names())
def test_case_table_single_stream_and_batch(ctx, oracle, name):
    """loudnorm_push / loudnorm_drain (lnb_limiter_kernel for the one stream of a single context) against the oracle and the
    recorded hashes, then loudnorm_process_batch holding the case as stream 2 of 4, bit-identical to the single-stream context"""
    case = LC.get(name)
    try:
        single, exp = _case_single(oracle, case)
        n_diff, rel = int((single != exp).sum()), _close(single, exp)
        print("%s: %d of %d samples differ from the oracle, scale-relative %.3g" % (name, n_diff, single.size, rel))
        assert single.size == case.x.size
        assert rel <= 1e-9
        if name.startswith("grid"):
            assert n_diff == 0
        if name != "len_3s_minus_1":
            assert np.abs(single).max() <= 10 ** (-2.0 / 20)
        late, prog, quiet = _fillers(case)
        got = _run_batch(ctx, [late, prog, case.x, quiet], case.channels, **case.kw)
        assert got.shape[1] == single.size
        assert (got[2] == single).all(), (name, int((got[2] != single).sum()))
        assert _close(got[2], exp) <= 1e-9
    finally:
        case.release()
