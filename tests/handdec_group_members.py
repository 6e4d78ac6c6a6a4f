"""The members of the hand-decoder queue's tests, shared by tests/test_group_handdec_cpu.py (the layout of the mixed set) and
tests/test_gpu_group_handdec.py (the set itself). Cases come from tests/handdec_cases.py's builders, so the near_tie assertion of
its case constructors is in force; nothing here touches a device."""
import numpy as np

import handdec_cases as H

PALM, LANDMARKS = 0, 1

# palm N; the job without rows sits between two with rows; the last one keeps no row (its threshold is above every score)
MIXED_PALM_N = [1, 63, 64, 0, 65, 255, 256, 257, 1023, 1024, 1025, 2016, 4096, 300]
# landmarks (H, D, scores): absent, fewer than H ("short"), at least H ("full")
MIXED_LANDMARKS = [(1, 2, "absent"), (3, 3, "short"), (0, 3, "absent"), (4, 16, "full"), (5, 2, "full"), (10, 3, "absent"), (11, 16, "short"), (64, 3, "full"),
                   (7, 2, "short")]


def mixed_spec():
    """[(decoder, rows, D, scores kind)] in submit order: palm and landmark jobs interleaved."""
    out, p, l = [], list(MIXED_PALM_N), list(MIXED_LANDMARKS)
    while p or l:
        if p:
            out.append((PALM, p.pop(0), 0, None))
        if l:
            h, d, kind = l.pop(0)
            out.append((LANDMARKS, h, d, kind))
    return out


def palm_settings(k):
    rng = np.random.default_rng(140 + k)
    return (float(rng.uniform(0.0, 0.8)), float(rng.uniform(0.0, 0.6)), 1 + k % 8, H.FRAMES[k % 3])


def landmark_settings(k):
    rng = np.random.default_rng(160 + k)
    return (float(rng.uniform(0.2, 0.8)), float(rng.uniform(-0.1, 0.6)), 1 + k % 10, H.FRAMES[k % 3])


def palm_case(k, N, params=None):
    data = H.palm_synth(5000 + k, N)
    if N == 1:
        data[0] = (0.9, 0.5, 0.5, 0.2, 0.5, 0.6, 0.5, 0.5)    # valid: the lone row is a hand
    return H.PalmCase("m%d_palm_N%d" % (k, N), data, params or palm_settings(k))


def landmark_case(k, Hn, D, kind, params=None):
    rng = np.random.default_rng(6000 + k)
    data = H.hand_synth(rng, Hn, D)
    scores = None if kind == "absent" else rng.uniform(0, 1, max(Hn // 2, 1) if kind == "short" else Hn + 3).astype(np.float32)
    return H.LandmarkCase("m%d_landmarks_H%d_D%d_%s" % (k, Hn, D, kind), data, scores, params or landmark_settings(k))


def mixed_cases():
    cases = []
    for k, (decoder, rows, D, kind) in enumerate(mixed_spec()):
        if decoder == PALM:
            p = (5.0, 0.3, 8, None) if rows == 300 else (-1.0, 0.0, 3, (640, 360)) if rows == 1 else None    # no survivor / the lone row survives
            cases.append(palm_case(k, rows, p))
        else:
            cases.append(landmark_case(k, rows, D, kind))
    return cases
