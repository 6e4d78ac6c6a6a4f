"""The sampling cadence of the run-time kernel choice (csrc/autopick.hpp) when the input's provenance settles the question: a
launch that reads what the launch before it wrote, still on-die (hsvfilter ! colorlut), with the table kind in use. Driven on a
scripted device through mi355_selftest_autopick_settled - no GPU needed; tests/test_autopick.py holds the policy's other rules,
which this cadence leaves alone (the last test here runs one of its scripts through both hooks)."""
import ctypes as C

import numpy as np

NV = 16_588_800  # pixel groups of an 8 x 4K launch: sampled every 8th launch where the cadence does not thin out


def run(mi355lib, n, ms_c, ms_t, settled, lag=0, nv=NV):
    a = (C.c_double * n)(*[float(v) for v in ms_c])
    b = (C.c_double * n)(*[float(v) for v in ms_t])
    s = (C.c_int * n)(*[int(v) for v in settled]) if settled is not None else None
    kind, meas = (C.c_int * n)(), (C.c_int * n)()
    assert mi355lib.mi355_selftest_autopick_settled(n, (C.c_uint64 * n)(*[nv] * n), a, b, s, lag, kind, meas) == 0
    return np.array(kind[:]), np.array(meas[:])


def samples_in_use(kind, meas, start=20):
    """launches of the table kind that were measured, after the learning phase (four measurements, each read back `lag` <= 3
    launches late); a probe's measured half runs the other kind"""
    return [i for i in range(start, len(kind)) if meas[i] and kind[i] == 1]


def test_settled_input_thins_the_samples_out_to_one_per_1024(mi355lib):
    n = 6000
    kind, meas = run(mi355lib, n, [0.25] * n, [0.12] * n, [1] * n, lag=3)
    s = samples_in_use(kind, meas)
    gaps = np.diff(s)
    assert gaps[0] <= 64 and all(b >= a for a, b in zip(gaps, gaps[1:])), gaps            # short first, never shorter again
    assert sum(1 for g in gaps if g >= 1024) >= 3, gaps                                   # the period reaches 1024 and stays
    assert max(gaps) <= 1024 + 3 + 2, gaps                                                # the top of the ladder, + read-back lag and a probe's two launches
    assert len(s) <= 14                                                                   # 8, 16, ... 1024: eight steps, then one per 1024
    # the every-8th cadence of the same script without the provenance: two orders of magnitude more markers in the stream
    kind0, meas0 = run(mi355lib, n, [0.25] * n, [0.12] * n, [0] * n, lag=3)
    assert len(samples_in_use(kind0, meas0)) >= n // 8 - 40
    # the other kind is still asked on its own ladder, two launches at a time (a probe waits while a sample is in flight: a few launches' shift)
    other, other0 = ([i for i in range(20, n) if k[i] == 0] for k in (kind, kind0))
    assert other and len(other) % 2 == 0 and len(other) == len(other0) and all(abs(a - b) <= 8 for a, b in zip(other, other0)), (other, other0)


def test_a_30_percent_change_brings_the_probe_forward_at_the_next_sample(mi355lib):
    n, change = 6000, 3000
    ms_t = [0.12] * change + [0.156] * (n - change)          # the table kernel 30 % slower: still ahead of 0.25, the choice stays
    kind, meas = run(mi355lib, n, [0.25] * n, ms_t, [1] * n, lag=3)
    s = samples_in_use(kind, meas)
    before = [i for i in s if i < change]
    assert before[-1] - before[-2] >= 1024                   # the cadence had reached the top of the ladder
    first = next(i for i in s if i >= change)                # the next sample, whenever the ladder has it
    assert first - before[-1] <= 1024 + 3 + 2
    probe = [i for i in range(first, n) if kind[i] == 0][:2]
    # ... is read back `lag` launches later and the other kind is asked at once: two launches, the second measured
    assert probe and probe[0] - first <= 3 + 2 and probe[1] == probe[0] + 1 and meas[probe[0]] == 0 and meas[probe[1]] == 1, (first, probe)
    # without the change that probe would have waited for the long period
    kind1, _ = run(mi355lib, n, [0.25] * n, [0.12] * n, [1] * n, lag=3)
    assert not [i for i in range(first, probe[1] + 50) if kind1[i] == 0]
    # and the kind in use is watched closely again: the cadence starts over at every 8th launch
    after = [i for i in s if i > first]
    assert after[0] - first <= 8 + 3 + 2 and after[1] - after[0] <= 16 + 3, (first, after[:4])


def test_provenance_that_comes_and_goes_keeps_the_short_cadence(mi355lib):
    """The ladder belongs to a run of settled launches: a launch from HBM in between returns the cadence to every 8th."""
    n = 2000
    settled = [0 if i % 50 == 49 else 1 for i in range(n)]
    kind, meas = run(mi355lib, n, [0.25] * n, [0.12] * n, settled, lag=1)
    gaps = np.diff(samples_in_use(kind, meas))
    assert max(gaps) <= 50 + 8


def test_without_provenance_nothing_changes(mi355lib):
    """settled = NULL and settled = all zero are mi355_selftest_autopick, call by call."""
    n = 1500
    rng = np.random.default_rng(3)
    ms_c = 0.2 * (1 + rng.uniform(-0.3, 0.3, n))
    ms_t = 0.2 * (1 + rng.uniform(-0.3, 0.3, n))
    kind = (C.c_int * n)()
    meas = (C.c_int * n)()
    nv = (C.c_uint64 * n)(*[NV] * n)
    a, b = (C.c_double * n)(*ms_c), (C.c_double * n)(*ms_t)
    assert mi355lib.mi355_selftest_autopick(n, nv, a, b, 2, kind, meas) == 0
    for settled in (None, [0] * n):
        k2, m2 = run(mi355lib, n, ms_c, ms_t, settled, lag=2)
        assert (k2 == np.array(kind[:])).all() and (m2 == np.array(meas[:])).all()
