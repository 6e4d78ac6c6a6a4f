"""CPU tests of audioloudnorm's two CPU readings of imp.rs against each other, branch by branch.

oracle/loudnorm_oracle.c is what the device is compared with (tests/test_gpu_loudnorm.py); tests/loudnorm_restate.py is a second
restatement written from imp.rs alone. With the same meters and unfused arithmetic on both sides their outputs are equal
BIT FOR BIT on every case of tests/loudnorm_cases.py; every case reaches the limiter branches it claims; the union of the
traces covers every label of the restatement's table but the ones argued unreachable there; and the oracle runs the
cases whose final call crosses the ring's end clean under the host's AddressSanitizer."""
import os
import random
import subprocess

import numpy as np
import pytest

import loudnorm_cases as LC
import loudnorm_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_RESULTS = {}


def _oracle_run(oracle, case):
    ln = oracle.LoudNorm(case.channels, **case.kw)
    outs = [ln.push(part) for part in case.chunks()]
    d = ln.drain()
    assert d is not None
    return np.concatenate(outs + [d])


def _restate_run(oracle, case, **kw):
    st = R.State(oracle, case.channels, **dict(case.kw, **kw))
    outs = [st.push(part) for part in case.chunks()]
    d = st.drain()
    assert d is not None
    return st, np.concatenate(outs + [d])


def _result(oracle, name):
    """(restatement state, restatement output, oracle output, strict-mode exception or None), once per case and session"""
    if name not in _RESULTS:
        case = LC.get(name)
        strict_error = None
        if case.strict_ok:
            st, got = _restate_run(oracle, case, element_wrap=False)   # the reference's own walk: never leaves the ring here
        else:
            try:
                _restate_run(oracle, case, element_wrap=False)
            except R.RingOverrun as e:
                strict_error = e
            st, got = _restate_run(oracle, case, element_wrap=True)
        exp = _oracle_run(oracle, case)
        case.release()
        _RESULTS[name] = (st, got, exp, strict_error)
    return _RESULTS[name]


@pytest.mark.parametrize("name", LC.names())
def test_restatement_equals_oracle_bit_for_bit(oracle, name):
    st, got, exp, _ = _result(oracle, name)
    case = LC.get(name)
    assert got.shape == exp.shape
    assert got.tobytes() == exp.tobytes(), (name, int((got != exp).sum()), float(np.abs(got - exp).max()))
    tp = 10.0 ** (case.kw.get("max_true_peak", -2.0) / 20.0)
    if "frame.linear" not in st.trace:
        assert np.abs(got).max() <= tp


@pytest.mark.parametrize("name", LC.names())
def test_case_reaches_the_branches_it_claims(oracle, name):
    st, _, _, _ = _result(oracle, name)
    missing = [l for l in LC.get(name).claims if l not in st.trace]
    assert not missing, (name, missing, sorted(st.trace))


def test_every_label_is_reached_by_some_case(oracle):
    assert set(R.UNREACHABLE) <= set(R.LABELS)
    for label, why in R.UNREACHABLE.items():
        assert label.startswith("att."), "only an Attack label may be exempt"
        assert "imp.rs" in why and len(why) > 200
    union = set()
    for name in LC.names():
        union |= _result(oracle, name)[0].trace
    assert not (union & set(R.UNREACHABLE)), "an exempt label was reached: the argument is wrong"
    assert set(R.LABELS) - union - set(R.UNREACHABLE) == set()
    claimed = {l for c in LC.all_cases() for l in c.claims}
    assert set(R.LABELS) - claimed - set(R.UNREACHABLE) == set(), "every label is CLAIMED by a case, not only met by chance"


def test_unreachable_clamp_argument_holds(oracle):
    """att.higher_shallower_clamped: every entry to the shallower-slope branch has g0 > g1 > gain_reduction, and the quotient of
    two correctly rounded differences a >= b > 0 is never below 1.0 (checked on the entries and on adjacent doubles)"""
    entries = []
    for name in LC.names():
        entries += _result(oracle, name)[0].shallow_entries
    assert len(entries) >= 5
    for g0, g1, r in entries:
        assert g0 > g1 > r > 0.0
        assert (r - g0) / -(g0 - g1) >= 1.0
    rng = random.Random(7)
    for _ in range(20000):
        g1 = rng.uniform(0.01, 0.99)
        g0 = g1 + rng.choice([rng.uniform(0.0, 1.0 - g1), 10.0 ** rng.uniform(-16, -3)])
        if not g0 > g1:
            continue
        r = g1
        for _ in range(rng.randint(1, 3)):
            r = np.nextafter(r, 0.0)
        assert (float(r) - g0) / -(g0 - g1) >= 1.0


@pytest.mark.parametrize("name", [n for n in LC.names() if n.startswith("misaligned")])
def test_misaligned_final_call_index_trace(oracle, name):
    """the last call of these streams starts at an index that is no multiple of `channels`, and multiplies frames; the in-bounds
    ones pass the reference's own frame-wise walk, the crossing ones leave the ring with it (the restatement raises there) and
    are defined by the element-wise wrap only"""
    st, _, _, strict_error = _result(oracle, name)
    case, last = LC.get(name), st.calls[-1]
    ch, llen = case.channels, (2 * R.FRAME_SIZE + R.LIMITER_LOOKAHEAD) * case.channels
    print(name, {k: last[k] for k in ("call", "nb", "index", "misaligned_by", "state_in", "state_out")}, "ring", llen, last["labels"])
    assert last["frame_type"] == R.FINAL and last["nb"] == len(case.x) % R.FRAME_SIZE and last["nb"] < R.FRAME_SIZE
    case.release()
    assert (R.FRAME_SIZE - last["nb"]) % ch != 0 and last["misaligned_by"] == last["index"] % ch != 0
    assert "final.misaligned_writes" in last["labels"]
    assert all(c["misaligned_by"] == 0 for c in st.calls[:-1])
    crossing = [l for l in last["labels"] if l.startswith("final.crossing")]
    if case.strict_ok:
        assert strict_error is None and not crossing
    else:
        assert isinstance(strict_error, R.RingOverrun) and crossing


@pytest.mark.parametrize("name", ["grid_plateau", "misaligned_crossing_2ch"])
def test_literal_loops_equal_the_numpy_ones(oracle, name):
    """fast=False: every fill, the output copy and detect_peak as the serial loops of imp.rs"""
    _, got, _, _ = _result(oracle, name)
    case = LC.get(name)
    st, lit = _restate_run(oracle, case, element_wrap=not case.strict_ok, fast=False)
    case.release()
    assert lit.tobytes() == got.tobytes()
    assert st.trace == _result(oracle, name)[0].trace


def test_detect_peak_serial_equals_vectorised_on_random_rings(oracle):
    """random rings quantised to a few levels (plateaus of equal samples above and below the ceiling everywhere), random start,
    aligned and misaligned with the element-wise wrap: same result and same carried prev_smp"""
    rng = np.random.default_rng(11)
    hits = plateaus = 0
    for trial in range(200):
        ch = int(rng.choice([1, 2, 3, 6]))
        a, b = R.State(oracle, ch, element_wrap=True, fast=False), R.State(oracle, ch, element_wrap=True, fast=True)
        frames = a.limiter_buf.size // ch
        v = rng.choice([0.1, 0.3, 0.5, 0.78, 0.85, 0.9, 1.0, 1.2], (frames, ch), p=[0.3, 0.25, 0.2, 0.05, 0.05, 0.05, 0.05, 0.05])
        keep = rng.random((frames, ch)) < 0.4                      # repeat the previous frame's value: runs of equal samples
        src = np.maximum.accumulate(np.where(keep, 0, np.arange(frames)[:, None]), axis=0)
        ring = (np.take_along_axis(v, src, axis=0) * rng.choice([-1.0, 1.0], (frames, ch))).reshape(-1)
        lbi = int(rng.integers(0, ring.size))
        if trial % 2 == 0:
            lbi -= lbi % ch
        prev = [float(v) for v in rng.uniform(0.0, 1.0, ch)]
        offset, samples = int(rng.integers(0, 19000)), int(rng.integers(0, 400))
        for s in (a, b):
            s.limiter_buf[:] = ring
            s.limiter_buf_index = lbi
            s.prev_smp = list(prev)
            s.calls.append({})
        ra, rb = a.detect_peak(offset, samples), b.detect_peak(offset, samples)
        assert ra == rb, (trial, ra, rb)
        assert a.prev_smp == b.prev_smp or samples == 0, trial
        hits += ra is not None
        plateaus += "dp.plateau" in a.trace and "dp.plateau" in b.trace
    assert hits > 100 and plateaus > 30, (hits, plateaus)


def test_strict_mode_raises_on_a_straddling_frame(oracle):
    st = R.State(oracle, 2, element_wrap=False)
    st.calls.append({})
    with pytest.raises(R.RingOverrun):
        st._mul_frame(st.limiter_buf.size - 1, 0.5)
    st2 = R.State(oracle, 2, element_wrap=True)
    st2.calls.append({})
    st2.limiter_buf[-1], st2.limiter_buf[0] = 2.0, 4.0
    assert st2._mul_frame(st2.limiter_buf.size - 1, 0.5) == 1
    assert st2.limiter_buf[-1] == 1.0 and st2.limiter_buf[0] == 2.0


# ---------------------------------------------------------------- the oracle under the host's AddressSanitizer

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def asan_driver(tmp_path_factory):
    """tests/cpu_replay/loudnorm_asan_driver.c + the oracle's loudnorm and ebur128 sources as one sanitized executable.
    Skips only if an empty program does not build with the sanitizer flags."""
    d = tmp_path_factory.mktemp("loudnorm_asan")
    empty = d / "empty.c"
    empty.write_text("int main(void) { return 0; }\n")
    static = ["-static-libasan"]      # the runtime inside the executable: nothing has to be loaded ahead of it
    if subprocess.call(["gcc"] + SAN + static + ["-o", str(d / "empty"), str(empty)], stderr=subprocess.DEVNULL) != 0:
        static = []
        if subprocess.call(["gcc"] + SAN + ["-o", str(d / "empty"), str(empty)], stderr=subprocess.DEVNULL) != 0:
            pytest.skip("the host compiler has no AddressSanitizer / UBSan")
    exe = d / "loudnorm_asan_driver"
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math"] + SAN + static +
                          ["-I", os.path.join(ROOT, "oracle"), "-o", str(exe), os.path.join(HERE, "cpu_replay", "loudnorm_asan_driver.c"),
                           os.path.join(ROOT, "oracle", "loudnorm_oracle.c"), os.path.join(ROOT, "oracle", "ebur128_oracle.c"), "-lm"])
    return str(exe)


# (channels, frames): (19200 - frames % 19200) % channels != 0 and the short call's walk crosses the ring's end (index trace of
# test_misaligned_final_call_index_trace); 931200 is the aligned neighbour
@pytest.mark.parametrize("ch,frames", [(2, 931201), (2, 892801), (2, 610201), (3, 610201), (6, 610201), (2, 931200), (3, 604801)])
def test_oracle_is_clean_under_address_sanitizer(asan_driver, ch, frames):
    p = subprocess.run([asan_driver, str(ch), str(frames)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.stdout.startswith("frames_out %d " % frames)
