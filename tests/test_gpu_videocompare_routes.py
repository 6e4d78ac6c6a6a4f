"""GPU replay of tests/videocompare_cases.py: videocompare's five hash kernels branch by branch at the smallest frames, through the
device entry (mi355_videocompare_hash_frames_device) on poisoned buffers, and through the host entry where a case says so. Every
hash == the C oracle's, bit for bit (integer sums, order-pinned f32); cases that hash the same pixels through different kernels
also equal each other. tests/test_videocompare_cases_cpu.py proves that each case reaches the branch it is here for."""
import pytest

import videocompare_cases as V

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _device(ctx, case, algo="blockhash", lead=None):
    """The case's frames on the device in their poisoned buffer, hashed in one call at base + lead."""
    lead = case.lead if lead is None else lead
    frames = case.frames()
    buf = V.pack(frames, case.width, case.height, case.channels, case.stride, case.pitch, lead)
    d = ctx.alloc(buf.size + 16)
    try:
        assert d % 16 == 0
        ctx.h2d(d, buf)
        got = ctx.videocompare_hash_frames_device(d + lead, case.pitch, case.stride, case.n_frames, case.width, case.height, case.fmt, algo)
    finally:
        ctx.free(d)
    return frames, got


def _oracle(oracle, case, frames):
    return [oracle.blockhash(f, case.width, case.height, case.width * case.channels, case.channels) for f in frames]


@pytest.fixture(scope="module")
def r1_hashes(mi355lib):
    """R1 (the vector kernel on padded rows with a frame gap), once for R2..R4 to compare with; R1's own case holds it to the oracle."""
    import mi355fx
    with mi355fx.Context(0) as c:
        return _device(c, V.ROUTE_CASES[0])[1]


@pytest.mark.parametrize("case", V.ROUTE_CASES, ids=_ids(V.ROUTE_CASES))
def test_routes(ctx, oracle, r1_hashes, case):
    frames, got = _device(ctx, case)
    assert got == _oracle(oracle, case, frames)
    assert len(set(got)) == case.n_frames
    if case.pixels == "R1":
        assert got == r1_hashes                       # the same pixels through the bytes kernel
    if case.pixels == "R6":
        assert got == _device(ctx, V.ROUTE_CASES[-2])[1]
    if not case.padded:                                # the host entry repacks every frame to a 16-byte pitch
        assert [ctx.videocompare_hash_frame(f, case.width * case.channels, case.width, case.height, case.fmt) for f in frames] == got


@pytest.mark.parametrize("case", V.SPLIT_CASES, ids=_ids(V.SPLIT_CASES))
def test_lane_split(ctx, oracle, case):
    frames, got = _device(ctx, case)
    exp = _oracle(oracle, case, frames)
    assert got == exp
    assert _device(ctx, case, lead=4)[1] == exp        # the same pixels 4 bytes off: one lane per pixel


@pytest.mark.parametrize("case", V.LADDER_CASES, ids=_ids(V.LADDER_CASES))
def test_several_frames_per_workgroup(ctx, oracle, case):
    frames, got = _device(ctx, case)
    exp = _oracle(oracle, case, frames)
    bad = [k for k in range(case.n_frames) if got[k] != exp[k]]
    assert bad == []
    assert all(exp[k] != exp[k + 1] for k in range(case.n_frames - 1))     # neighbours differ: a leak between them would show


@pytest.mark.parametrize("case", V.FINISH_CASES, ids=_ids(V.FINISH_CASES))
def test_finish_rule(ctx, oracle, case):
    frames, got = _device(ctx, case)
    assert got == _oracle(oracle, case, frames)
    assert got == [V.blockhash_bits(s, case.area) for s in case.claims["sums"](765 * case.area // 2, case.area)]
    if case.claims["literals"] is not None:
        assert got == case.claims["literals"]
    if case.kernel == "vec":
        assert _device(ctx, case, lead=4)[1] == got    # the bytes kernel's sums, the same finish


@pytest.mark.parametrize("case", V.ANY_SIZE_CASES, ids=_ids(V.ANY_SIZE_CASES))
def test_any_size(ctx, oracle, case):
    import mi355fx
    with pytest.raises(mi355fx.Mi355Error) as e:
        _device(ctx, case)
    assert e.value.status == mi355fx.ERR_UNSUPPORTED
    ctx.set_flag(mi355fx.FLAG_BLOCKHASH_ANY_SIZE, 1)
    frames, got = _device(ctx, case)
    assert got == _oracle(oracle, case, frames)
    assert got == [V.any_size_bits(f, case.width, case.height, case.channels) for f in frames]
    assert [ctx.videocompare_hash_frame(f, case.width * case.channels, case.width, case.height, case.fmt) for f in frames] == got


@pytest.mark.parametrize("case", V.RESIZE_CASES, ids=_ids(V.RESIZE_CASES))
def test_resize_based_hashes(ctx, oracle, case):
    w, h, c = case.width, case.height, case.channels
    for algo, bits in V.ALGOS:
        frames, got = _device(ctx, case, algo)
        exp = [oracle.imghash(f, w, h, w * c, c, algo) for f in frames]
        assert [e[1] for e in exp] == [bits] * 3
        assert [hex(g) for g in got] == [hex(e[0]) for e in exp], algo
        assert [ctx.videocompare_hash_frame(f, w * c, w, h, case.fmt, algo) for f in frames] == got, algo     # the host entry, frame by frame


@pytest.mark.parametrize("algo,a,b,literal", V.DISTANCE_CASES, ids=["all-64", "top-bit", "doublegradient-40"])
def test_distance(ctx, oracle, algo, a, b, literal):
    got = ctx.videocompare_distance(a, b, algo)
    assert got == oracle.hash_distance(a, b)
    if literal is not None:
        assert got == literal
