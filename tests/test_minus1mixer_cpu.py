"""minus1mixer / audiomultimixer without a GPU: the restatement's known answers (tests/minus1mixer_restate.py: the reference's own
1 / 10 / 100 vectors and hand-worked values), the host-only planner behind the kernel's job table (mi355_selftest_mixer_plan) and
the ABI surface of the new entry points."""
import ctypes as C
import re

import numpy as np
import pytest

import minus1mixer_cases as M
import minus1mixer_restate as R

F32, S16 = R.F32, R.S16


# ---------------------------------------------------------------- restatement: known answers

@pytest.mark.parametrize("fmt", [F32, S16], ids=["F32", "S16"])
def test_reference_vectors_1_10_100(fmt):
    """minus1mixer_direct_link_* (audio/audiomultimixer/src/tests/minus1mixer.rs:146-291): 110, 101, 11 exactly"""
    case = M.reference_vectors(fmt, fmt)
    for out, want in zip(case.expected(), (110, 101, 11)):
        assert out.dtype == R.DTYPE[fmt] and out.shape == (M.FRAMES,) and (out == want).all()


def test_reference_vectors_across_formats():
    for i, o in ((S16, F32), (F32, S16)):
        case = M.reference_vectors(i, o)
        for out, want in zip(case.expected(), M.reference_answer(i, o)):
            assert (out == want).all(), (i, o)


@pytest.mark.parametrize("name,values,f32_bits,s16", M.SPECIALS, ids=[s[0] for s in M.SPECIALS])
def test_hand_worked_values(name, values, f32_bits, s16):
    f, s = M.special_case(values).expected()
    if f32_bits is None:
        assert np.isnan(f[0])
    else:
        assert int(f.view(np.uint32)[0]) == f32_bits, hex(int(f.view(np.uint32)[0]))
    assert int(s[0]) == s16


def test_order_is_part_of_the_result():
    a = M.special_case(np.array([1e8, 1.0, -1e8], np.float32)).expected()[0][0]
    b = M.special_case(np.array([1e8, -1e8, 1.0], np.float32)).expected()[0][0]
    assert a == 0.0 and b == 1.0


def test_one_participant_hears_silence():
    for fmt in (F32, S16):
        case = M.Case(R.minus1(1), [(0, M.samples(np.random.default_rng(3), fmt, 50), 0)], [(F32, 0, 1), (S16, 0, 1)], 50)
        f, s = case.expected()
        assert not f.view(np.uint32).any() and not s.any()


def test_a_channel_nobody_feeds_is_silence():
    case = M.random_general(5, 4, 6, 33)
    silent = 6 // 2
    assert not case.contrib[:, silent].any()
    assert case.outputs[0] == (S16, silent, 1) and case.outputs[1] == (F32, silent, 1)
    s, f = case.expected()[:2]
    assert not s.any() and not f.view(np.uint32).any()


def test_segments_land_at_their_offset_and_gaps_stay_silent():
    x = np.array([1, 2, 3], np.float32)
    case = M.Case(np.ones((2, 1), bool), [(0, x, 2), (1, x[:2], 4), (0, x[:0], 0)], [(F32, 0, 1)], 8)
    assert case.expected()[0].tolist() == [0, 0, 1, 2, 4, 2, 0, 0]


def test_interleaved_outputs():
    a, b = np.array([1, 2], np.float32), np.array([10, 20], np.float32)
    contrib = np.array([[1, 0, 1], [0, 1, 1]], bool)
    case = M.Case(contrib, [(0, a, 0), (1, b, 0)], [(F32, 0, 2), (F32, 1, 2)], 2)
    o0, o1 = case.expected()
    assert o0.tolist() == [1, 10, 2, 20] and o1.tolist() == [10, 11, 20, 22]


# ---------------------------------------------------------------- the planner

MEMBERS = [(1, 1, 1), (3, 3, 480), (64, 64, 481), (256, 256, 7), (5, 2, 0)]   # (n_inputs, n_out_channels, frames)
GROUP = 16   # output channels per block (csrc/mixer.hip: kMixGroup)


def _plan(lib, members, n_segments=None, n_outputs=None, with_blocks=True):
    n = len(members)
    u32, u64 = C.c_uint32, C.c_uint64
    arr = lambda t, v: (t * max(len(v), 1))(*v)
    ni, nc = arr(u32, [m[0] for m in members]), arr(u32, [m[1] for m in members])
    ns = arr(u32, n_segments or [m[0] + 1 for m in members])
    no = arr(u32, n_outputs or [m[1] for m in members])
    fr = arr(u64, [m[2] for m in members])
    fb, so, oo, bo = ((u32 * (n + 1))() for _ in range(4))
    rc = lib.mi355_selftest_mixer_plan(n, ni, nc, ns, no, fr, fb, so, oo, bo, 0, None, None, None)
    if rc or not with_blocks:
        return rc, None
    total = fb[n]
    bm, bt, bg = ((u32 * max(total, 1))() for _ in range(3))
    rc = lib.mi355_selftest_mixer_plan(n, ni, nc, ns, no, fr, fb, so, oo, bo, total, bm, bt, bg)
    return rc, dict(first_block=list(fb), seg=list(so), out=list(oo), bits=list(bo), member=list(bm)[:total], tile=list(bt)[:total], group=list(bg)[:total])


def test_binding_and_header_agree_on_the_frame_tile():
    import mi355fx
    m = re.search(r"#define\s+MI355_MIXER_FRAME_TILE\s+(\d+)", open(mi355fx.HEADER_PATH).read())
    assert m and int(m.group(1)) == mi355fx.MIXER_FRAME_TILE


def test_plan_every_sample_has_exactly_one_block(mi355lib):
    import mi355fx
    T = mi355fx.MIXER_FRAME_TILE
    rc, p = _plan(mi355lib, MEMBERS)
    assert rc == 0
    fb = p["first_block"]
    assert fb[0] == 0 and fb[-1] == len(p["member"]) and all(a <= b for a, b in zip(fb, fb[1:]))
    owners = [np.zeros((m[2], m[1]), np.int32) for m in MEMBERS]
    for b, (j, t, g) in enumerate(zip(p["member"], p["tile"], p["group"])):
        assert fb[j] <= b < fb[j + 1], "block %d crosses a member" % b
        n_in, n_out, frames = MEMBERS[j]
        assert t * T < frames and g * GROUP < n_out, (b, j, t, g)
        owners[j][t * T:(t + 1) * T, g * GROUP:(g + 1) * GROUP] += 1
    for j, o in enumerate(owners):
        assert (o == 1).all(), j
    assert fb[4] == fb[5], "a member without frames gets no block"
    assert fb[1] - fb[0] == 1 and fb[2] - fb[1] == 8 and fb[3] - fb[2] == 8 * 4 and fb[4] - fb[3] == 16


def test_plan_table_offsets_are_running_sums_within_bounds(mi355lib):
    n_segments, n_outputs = [0, 5, 1024, 300, 2], [1, 3, 70, 512, 0]
    rc, p = _plan(mi355lib, MEMBERS, n_segments, n_outputs)
    assert rc == 0
    words = [m[0] * -(-m[1] // GROUP) for m in MEMBERS]
    for key, sizes in (("seg", n_segments), ("out", n_outputs), ("bits", words)):
        off = p[key]
        assert off[0] == 0 and off[-1] == sum(sizes)
        for j, size in enumerate(sizes):
            assert off[j + 1] - off[j] == size and off[j] + size <= off[-1], (key, j)


def test_plan_refuses_what_is_beyond_the_limits(mi355lib):
    import mi355fx
    ok = (3, 3, 480)
    assert _plan(mi355lib, [ok, (256, 256, 1 << 20)], with_blocks=False)[0] == 0
    for bad in ((257, 3, 480), (3, 257, 480), (3, 3, (1 << 20) + 1)):
        assert _plan(mi355lib, [ok, bad], with_blocks=False)[0] == mi355fx.ERR_UNSUPPORTED, bad
    assert _plan(mi355lib, [ok], n_segments=[1025], with_blocks=False)[0] == mi355fx.ERR_UNSUPPORTED
    assert _plan(mi355lib, [ok], n_segments=[1024], with_blocks=False)[0] == 0
    assert _plan(mi355lib, [ok], n_outputs=[1025], with_blocks=False)[0] == mi355fx.ERR_UNSUPPORTED
    assert _plan(mi355lib, [ok], n_outputs=[1024], with_blocks=False)[0] == 0
    assert _plan(mi355lib, [(0, 3, 4)], with_blocks=False)[0] == mi355fx.ERR_INVALID_ARG
    assert _plan(mi355lib, [], with_blocks=False)[0] == 0


# ---------------------------------------------------------------- ABI surface

NEW_SYMBOLS = ("mi355_mixer_setup", "mi355_mixer_setup_minus1", "mi355_mixer_process", "mi355_mixer_process_device", "mi355_mixer_reset",
               "mi355_selftest_mixer_plan", "mi355_agroup_create_mixer", "mi355_agroup_shared_mixer", "mi355_agroup_mixer_setup",
               "mi355_agroup_mixer_setup_minus1", "mi355_agroup_submit_mixer", "mi355_agroup_mixer_launches")


def test_library_exports_the_entry_points(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and hasattr(mi355lib, name) and getattr(mi355lib, name).argtypes is not None, name
    assert mi355lib.mi355_abi_version() == 1


def test_structures_match_the_header_layout():
    import mi355fx
    assert C.sizeof(mi355fx.MixerSegment) == 24 and mi355fx.MixerSegment.input.offset == 8 and mi355fx.MixerSegment.num_frames.offset == 20
    assert C.sizeof(mi355fx.MixerOutput) == 24 and mi355fx.MixerOutput.format.offset == 8 and mi355fx.MixerOutput.n_channels.offset == 16


def test_header_names_the_refused_setup_calls():
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    para = hdr[hdr.index("A member's life cycle"):hdr.index("typedef struct mi355_agroup mi355_agroup;")]
    assert "mixer_setup" in para
