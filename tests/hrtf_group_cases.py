"""Member shapes and seeded block streams for the hrtfrender group tests (tests/test_gpu_agroup_hrtf.py, tests/test_agroup_hrtf_cpu.py)
and for the lone-path guard (tools/hrtf_lone_crc.py writes tests/golden/hrtf_lone_crc.json from the same streams).

Everything is generated from seeds on the mesh of tests/golden/test.hrir; nothing else is read."""
import os
import zlib

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESH = os.path.join(GOLDEN_DIR, "test.hrir")
CRC_FIXTURE = os.path.join(GOLDEN_DIR, "hrtf_lone_crc.json")

# (HRIR length L, channels C, interpolation-steps S, block-length B, method, expected transform size; 0 = the time-domain FIR)
SHAPES = [
    (256, 8, 8, 512, 0, 0),
    (512, 4, 2, 1500, 0, 2048),
    (400, 2, 8, 512, 0, 1024),
    (1, 1, 8, 512, 0, 0),          # the reference's fixture: one tap
    (2049, 2, 2, 2048, 0, 4096),
    (2050, 2, 2, 2048, 0, 0),      # window 4097: above the ceiling of the transform
    (128, 64, 8, 512, 1, 1024),
    (100, 3, 4, 77, 2, 0),
]
# the ninth member: a 200-tap sphere written at 44.1 kHz loaded into a 48 kHz member (218 taps after the resampling at load)
RESAMPLED = {"file_len": 200, "file_rate": 44100, "rate": 48000, "len": 218, "channels": 2, "steps": 8, "block": 512, "method": 0, "transform": 0}
RATE = 44100       # the rate the SHAPES spheres are written at and loaded at
GUARD_BLOCKS = 3   # blocks per shape in the lone-path guard


def mesh_bytes():
    with open(MESH, "rb") as f:
        return f.read()


def members():
    """every member of the heterogeneous set: dicts with key, sphere parameters, geometry, method and expected transform"""
    out = []
    for (L, C, S, B, method, n) in SHAPES:
        out.append({"key": "L%d_C%d_S%d_B%d_m%d" % (L, C, S, B, method), "file_len": L, "file_rate": RATE, "rate": RATE, "len": L, "channels": C,
                    "steps": S, "block": B, "method": method, "transform": n})
    out.append(dict(RESAMPLED, key="L200at44100_in48000_C2_S8_B512_m0"))
    return out


def sphere_bytes(synth, m, seed_offset=0):
    return synth.hrir_sphere_bytes(mesh_bytes(), m["file_len"], rate=m["file_rate"], seed=synth.SEED + 7 + seed_offset)


def stream(m, n_blocks, seed=0):
    """n_blocks of (input [S*B][C] f32, positions [C][3] f32, gains [C] f32): noise from moving sources, seeded by the shape"""
    C, frames = m["channels"], m["steps"] * m["block"]
    rng = np.random.default_rng(7919 * m["file_len"] + 31 * C + m["block"] + 1000003 * seed)
    pos = rng.standard_normal((C, 3)).astype(np.float32)
    out = []
    for _ in range(n_blocks):
        x = rng.uniform(-1, 1, (frames, C)).astype(np.float32)
        pos = (pos + 0.6 * rng.standard_normal((C, 3))).astype(np.float32)
        gains = rng.uniform(0.2, 1.0, C).astype(np.float32)
        out.append((x, pos.copy(), gains))
    return out


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def lone_context(mi355fx, synth, m, sphere=None):
    """a lone Context loaded and set up as member m (FLAG_HRTF_METHOD is read at setup)"""
    ctx = mi355fx.Context(0)
    ctx.hrtf_load_sphere(sphere if sphere is not None else sphere_bytes(synth, m), m["rate"])
    ctx.set_flag(mi355fx.FLAG_HRTF_METHOD, m["method"])
    try:
        ctx.hrtf_setup(m["channels"], m["block"], m["steps"])
    finally:
        ctx.set_flag(mi355fx.FLAG_HRTF_METHOD, 0)
    return ctx


def extra_members():
    """the members of the fixture's "extra" section (a reset after the first block; the device entry point), recorded later
    than the rest (at the commit the section names): the smallest member once per method, and - its single tap leaves a reset
    no tail to clear - one member per form whose tail a reset does clear"""
    small = members()[3]
    assert (small["len"], small["channels"]) == (1, 1)
    fft = dict(small, method=1, transform=512, key="L1_C1_S8_B512_m1")
    fir = dict(small, method=2, transform=0, key="L1_C1_S8_B512_m2")
    return [fft, fir, members()[2], members()[7]]


def lone_extra_crcs(mi355fx, synth, m):
    """GUARD_BLOCKS blocks twice: through the host entry point with a reset after the first block, and through
    hrtf_process_block_device on buffers the caller uploads and downloads itself"""
    frames, C = m["steps"] * m["block"], m["channels"]
    blocks = stream(m, GUARD_BLOCKS)
    ctx = lone_context(mi355fx, synth, m)
    try:
        reset = []
        for b, (x, p, g) in enumerate(blocks):
            if b == 1:
                ctx.hrtf_reset()
            reset.append(crc(ctx.hrtf_process_block(x, p, g)))
        n = ctx.hrtf_transform_size()
    finally:
        ctx.close()
    ctx = lone_context(mi355fx, synth, m)
    d_in, d_out = ctx.alloc(frames * C * 4), ctx.alloc(frames * 8)
    try:
        device = []
        for (x, p, g) in blocks:
            ctx.h2d(d_in, np.ascontiguousarray(x, np.float32))
            ctx.hrtf_process_block_device(d_in, d_out, p, g)   # (returns without waiting; the copy below is on the same stream)
            out = np.zeros(frames * 2, np.float32)
            ctx.d2h(out, d_out)
            device.append(crc(out))
        faces, uvw = ctx.hrtf_last_lookup()
        return {"transform": n, "reset": reset, "device": device, "faces": crc(faces.astype(np.int32)), "uvw": crc(uvw.astype(np.float32))}
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
        ctx.close()


def lone_crcs(mi355fx, synth, m):
    """CRC-32 of each of GUARD_BLOCKS output blocks of a lone context, and of the faces / weights of the last lookup"""
    ctx = lone_context(mi355fx, synth, m)
    try:
        outs = [crc(ctx.hrtf_process_block(x, p, g)) for (x, p, g) in stream(m, GUARD_BLOCKS)]
        faces, uvw = ctx.hrtf_last_lookup()
        return {"transform": ctx.hrtf_transform_size(), "out": outs, "faces": crc(faces.astype(np.int32)), "uvw": crc(uvw.astype(np.float32))}
    finally:
        ctx.close()
