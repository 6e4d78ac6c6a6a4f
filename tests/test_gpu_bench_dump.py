"""bench.py --dump-outputs on the GPU: the arrays written after the timed steps are what the last timed launch pair computed -
hsvfilter in place on the pristine source batch, then colorlut into the destination - checked against the CPU oracle, on the
sampled pixels and through every frame's per-channel sums."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dump_outputs_match_the_oracle(tmp_path, oracle, synth):
    import bench
    steps, warmup, pairs, nb = 2, 1, 4, 8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--ramp-seconds", "0.05",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("hsvfilter_out", "hsvfilter_out_channel_sums", "colorlut_out", "colorlut_out_channel_sums")}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the last timed pair's source batch: SourcePool index (warmup + steps) x pairs - 1, smooth content
    w, h = bench.W, bench.H
    index = (warmup + steps) * pairs - 1
    base = synth.smooth_frame(w, h, seed=synth.SEED + 17 * (index % 4))
    frames = np.ascontiguousarray(np.stack([np.roll(base, 4 * ((97 * i + 389 * (index // 4)) % w), axis=1) for i in range(nb)]))
    st = synth.HSV_SETTINGS["hue90"]
    cube = oracle.Cube.parse(synth.cube_text_3d(33))
    mid = frames.reshape(-1)
    oracle.hsvfilter(mid, w, w * 4, 4, 0, False, st, nthreads=16)
    mid = mid.reshape(nb, h * w * 4)
    out = np.zeros_like(mid)
    for i in range(nb):
        oracle.colorlut_rgba8(cube, mid[i], w * 4, out[i], w * 4, w, h, nthreads=16)
    mid, out = mid.reshape(nb, h * w, 4), out.reshape(nb, h * w, 4)

    k = bench.DUMP_SAMPLE_BYTES // (2 * nb * 4 * 4)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(h * w, size=k, replace=False))
    assert got["hsvfilter_out"].dtype == np.float32 and got["hsvfilter_out"].shape == (nb, k, 4)
    assert (got["hsvfilter_out"] == mid[:, idx]).all()
    assert (got["colorlut_out"] == out[:, idx]).all()
    assert got["hsvfilter_out_channel_sums"].dtype == np.float64
    assert (got["hsvfilter_out_channel_sums"] == mid.sum(axis=1)).all()
    assert (got["colorlut_out_channel_sums"] == out.sum(axis=1)).all()
