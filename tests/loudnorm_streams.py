"""The streams tests/test_gpu_loudnorm.py sends through loudnorm_push / loudnorm_drain of a single context, from one definition,
and the guard on their bits: tools/record_loudnorm_lone.py ran every one of them at the commit BEFORE the single context became a
batch of one (a second, host-driven implementation of the limiter then) and wrote the SHA-256 of each input and of each concatenated
output to tests/golden/loudnorm_lone_parent.json; the tests assert both inside the run they make anyway (`check`)."""
import hashlib
import json
import os

import numpy as np

import loudnorm_cases as LC

RATE = 192000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loudnorm_lone_parent.json")


def tone(seconds, ch, amp=0.02, f=440.0):
    t = np.arange(int(seconds * RATE)) / RATE
    return np.stack([amp * np.sin(2 * np.pi * (f + 3 * c) * t) for c in range(ch)], 1)


def burst_stream(seed, seconds, ch):
    """programme material with limiter work in it: a tone at a per-stream level with bursts far above the ceiling"""
    rng = np.random.default_rng(seed)
    x = tone(seconds, ch, amp=0.01 * (1 + seed % 5), f=300.0 + 37 * seed)
    for _ in range(6):
        i = int(rng.uniform(0.0, seconds - 0.05) * RATE)
        x[i:i + int(rng.integers(10, 3000))] *= rng.uniform(20.0, 90.0)
    return x + 1e-4 * rng.standard_normal(x.shape)


def limiter_heavy(ch):
    """Bursts far above the ceiling in every limiter situation: isolated, rising series (attack restarts), falling
    series (sustain), a burst inside the release window, one in the first 10 ms, one near the very end."""
    x = tone(7.3, ch)
    rng = np.random.default_rng(ch)
    for start, n, k in ((0.001, 40, 80.0), (3.5, 2000, 60.0), (3.52, 300, 90.0), (3.56, 100, 40.0), (3.7, 50, 30.0), (4.4, 10, 70.0),
                        (4.41, 10, 75.0), (4.42, 10, 85.0), (5.9, 500, 55.0), (7.28, 100, 65.0)):
        i = int(start * RATE)
        x[i:i + n] *= k
    x += 1e-4 * rng.standard_normal(x.shape)
    return x


def quiet_then_loud():
    return np.concatenate([tone(3.4, 2, amp=1e-6), tone(4.0, 2, amp=0.2), tone(1.1, 2, amp=0.01)])


def short_stream():
    return tone(1.3, 2, amp=0.05)


def exactly_three_seconds():
    x = tone(3.0, 1, amp=0.3)
    x[int(2.95 * RATE)] = 0.999
    return x


THREE_SECONDS_KW = dict(loudness_target=-16.0, loudness_range_target=11.0, max_true_peak=-1.0, offset=0.5)
BATCH_SHAPES = ((2, 5.23), (1, 3.0), (6, 3.71))   # test_batch_equals_separate_streams_and_oracle: (channels, seconds), 5 streams each


def batch_streams(ch, seconds):
    streams = [burst_stream(10 * ch + s, seconds, ch) for s in range(5)]
    streams[3] = tone(seconds, ch, amp=1e-6)           # below -70 LUFS throughout: above_threshold never set
    return streams


class Stream:
    """one guarded stream: `make()` -> (frames, channels) f64; `chunk`: frames per push (an int), or a case's list of push sizes
    (the rest in one piece; None: one push)"""

    def __init__(self, name, make, chunk, kw=None):
        self.name, self.make, self.chunk, self.kw = name, make, chunk, dict(kw or {})

    def parts(self, x):
        if isinstance(self.chunk, int):
            return [x[k:k + self.chunk] for k in range(0, len(x), self.chunk)]
        out, pos = [], 0
        for n in (self.chunk or []):
            out.append(x[pos:pos + n])
            pos += n
        if pos < len(x):
            out.append(x[pos:])
        return out


def streams():
    out = []
    for c in LC.all_cases():
        out.append(Stream("case/" + c.name, (lambda c=c: c.x), c.pushes, c.kw))
    for ch in (1, 2, 6):
        out.append(Stream("limiter_heavy/%dch" % ch, (lambda ch=ch: limiter_heavy(ch)), 123457))
    out.append(Stream("quiet_then_loud", quiet_then_loud, 96000))
    out.append(Stream("short_stream", short_stream, 50000))
    out.append(Stream("exactly_three_seconds", exactly_three_seconds, 192000, THREE_SECONDS_KW))
    for ch, seconds in BATCH_SHAPES:
        for s in range(5):
            out.append(Stream("batch_single/%dch/%d" % (ch, s), (lambda ch=ch, seconds=seconds, s=s: batch_streams(ch, seconds)[s]), 200000))
    return out


def get(name):
    for s in streams():
        if s.name == name:
            return s
    raise KeyError(name)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def run_lone(ctx, stream, x):
    """the stream through loudnorm_setup / _push / _drain of `ctx` -> the concatenated output"""
    ctx.loudnorm_setup(x.shape[1], **stream.kw)
    got = [ctx.loudnorm_push(p) for p in stream.parts(x)]
    d = ctx.loudnorm_drain()
    if d is not None:
        got.append(d)
    return np.concatenate(got)


_golden = None


def check(name, x, got):
    """`got`, the concatenated output of loudnorm_push / _drain for input `x`, is what the recorded commit gave for stream `name`"""
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)["streams"]
    rec, s = _golden[name], get(name)
    assert rec["chunk"] == s.chunk, (name, "pushed in other pieces than recorded")
    assert rec["input_sha256"] == sha(x), (name, "the input is not the recorded one")
    assert rec["output_sha256"] == sha(got), (name, "output differs from the recorded commit's")
