"""CPU proof of tests/videocompare_cases.py: every case reaches the branch it is in the table for, the numpy restatements agree with
the C oracle on every case, the literal hashes are what both give, and the poison in padding, gaps and lead bytes would show. No GPU."""
import numpy as np
import pytest

import videocompare_cases as V

FAST = V.ROUTE_CASES + V.SPLIT_CASES + V.LADDER_CASES + V.FINISH_CASES
BLOCKHASH = FAST + V.ANY_SIZE_CASES


def _ids(cases):
    return [c.id for c in cases]


def test_case_ids_are_unique():
    ids = _ids(BLOCKHASH + V.RESIZE_CASES)
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", BLOCKHASH, ids=_ids(BLOCKHASH))
def test_every_case_takes_the_kernel_it_claims(case):
    assert case.route() == case.kernel
    if not case.any_size:    # without the flag, and through the group, a frame of no whole blocks is refused
        return
    assert V.route(case.width, case.height, case.channels, case.stride, case.pitch, 0, case.n_frames, False) == "refused"
    assert V.route(case.width, case.height, case.channels, case.stride, None, 0, 1, True) == "refused"


def test_route_cases_leave_vec_by_one_term_each():
    """R2..R4 are R1 with one term of the predicate failed: mending that term alone gives vec again. R5 / R6 fail on width and on
    channels with every alignment term satisfied (but where the case says otherwise)."""
    r1, r2, r3, r4 = V.ROUTE_CASES[:4]
    assert (r1.stride % 16, r1.pitch % 16, r1.lead % 16) == (0, 0, 0) and r1.stride > r1.width * 4 and r1.pitch > r1.stride * r1.height
    assert (r2.stride % 16, r2.pitch % 16, r2.lead % 16) == (4, 0, 0)
    assert (r3.stride % 16, r3.pitch % 16, r3.lead % 16) == (0, 8, 0)
    assert (r4.stride % 16, r4.pitch % 16, r4.lead % 16) == (0, 0, 4)
    for c in (r2, r3, r4):
        assert c.pixels == r1.pixels and (c.width, c.height, c.channels, c.n_frames) == (r1.width, r1.height, r1.channels, r1.n_frames)
        assert (c.frames() == r1.frames()).all()
    for c in V.ROUTE_CASES[4:]:
        if c.claims["term"] == "width":
            assert c.width < 32 and c.channels == 4 and (c.stride % 16, c.pitch % 16, c.lead) == (0, 0, 0)
        else:
            assert c.channels == 3
    packed, padded = V.ROUTE_CASES[-2:]
    assert packed.stride % 16 != 0 and (padded.stride % 16, padded.pitch % 16) == (0, 0) and (packed.frames() == padded.frames()).all()
    widths = sorted(c.width for c in V.ROUTE_CASES if c.claims.get("term") == "width")
    assert widths == [8, 16, 24]


def test_only_r3_guards_the_pitch_term():
    """Without `frame_pitch % 16 == 0` in the predicate (the group path's form of it), R3 - and no other case of any table - would take
    the vector kernel and read uint4s 8 bytes off their alignment from the second frame on. That mutation is not run on a GPU: R3
    taking "bytes" and matching R1's hashes is the whole check."""
    flips = [c.id for c in FAST
             if V.route(c.width, c.height, c.channels, c.stride, None, c.lead % 16, c.n_frames, False) != c.route()]
    assert flips == ["R3-pitch+8"]
    r3 = V.ROUTE_CASES[2]
    assert r3.n_frames > 1 and (r3.pitch * 1) % 16 != 0 and (r3.pitch * 2) % 16 == 0     # frame 1 is misaligned, frame 2 is not


def test_lane_splits_are_each_pinned():
    assert [V.splits(w) for w in V.SPLIT_WIDTHS] == [{1, 2, 3}, {2}, {1, 2, 3}, {1, 2, 3}]
    assert set().union(*(V.splits(w) for w in V.SPLIT_WIDTHS)) == {1, 2, 3}
    assert [w // 8 for w in V.SPLIT_WIDTHS] == [5, 6, 7, 25]
    # the RGBA widths of test_gpu_videocompare.py but 200: block widths divisible by 4, no lane straddles
    assert all(V.splits(w) == set() for w in (64, 96, 320, 640, 1920, 3840))
    # split against a direct count of a lane's pixels in its first block column
    for w in V.SPLIT_WIDTHS + [1032, 2056]:
        bw = w // 8
        direct = {sum(1 for x in range(x0, x0 + 4) if x // bw == x0 // bw) for x0 in range(0, w, 4)}
        assert direct - {4} == V.splits(w)
    # every width ends its row in a wave that holds live and dead lanes
    for w in V.SPLIT_WIDTHS:
        assert 0 < V.live_lanes(w, 0) % 64 and V.live_lanes(w, 0) == w // 4


def test_split_heights_put_block_row_edges_where_they_claim():
    h8, h40, h264 = V.SPLIT_HEIGHTS
    assert h8 // 8 == 1                                                  # a block-row edge, and a flush, at every row
    groups = lambda h: [min(V.K_ROW_GROUP, h - y) for y in range(0, h, V.K_ROW_GROUP)]
    assert groups(h40) == [32, 8] and groups(h264) == [32] * 8 + [8]
    for h in (h40, h264):
        edges = range(h // 8, h, h // 8)
        assert any(y % V.K_ROW_GROUP != 0 for y in edges)                # an edge inside a row group
        assert any(y % V.K_ROW_GROUP % 8 != 0 for y in edges)            # ... and inside an unrolled run of 8 rows
    assert h264 // 8 == 33 and all(y % V.K_ROW_GROUP != 0 for y in range(33, 264, 33))   # no block-row edge on a row-group edge
    for c in V.SPLIT_CASES:
        assert c.stride % 16 == 0 and c.pitch % 16 == 0 and c.n_frames == 3


def test_long_rows_end_in_a_segment_of_two_live_lanes():
    for c in V.SPLIT_CASES[-2:]:
        segs = (c.width + V.VEC_SEG - 1) // V.VEC_SEG
        assert segs == c.claims["segments"]
        assert [V.live_lanes(c.width, s) for s in range(segs - 1)] == [256] * (segs - 1)
        live = V.live_lanes(c.width, segs - 1)
        assert live == c.claims["last_live"] == 2 and 0 < live < 64     # wave 0: lanes 0, 1 live, 62 dead; waves 1..3 all dead
        assert V.live_lanes(c.width, segs) == 0
        assert V.splits(c.width) == {1, 2, 3}                            # block widths 129, 257


@pytest.mark.parametrize("name,geom,rungs", V.LADDERS, ids=[l[0] for l in V.LADDERS])
def test_some_rung_crosses_frames_at_every_cu_count(name, geom, rungs):
    """Python cannot ask the library for the CU count: at every count from 1 to 512 some rung of the ladder has a workgroup whose
    items belong to more than one frame."""
    ipf = V.items_per_frame(geom["kernel"], geom["width"], geom["height"])
    assert ipf == {"vec": 3, "bytes": 8}[geom["kernel"]]
    missing = [n_cu for n_cu in range(1, 513) if not any(V.wg_crosses_frames(n, ipf, n_cu) for n in rungs)]
    assert missing == []
    assert not V.wg_crosses_frames(1, ipf, 256) and not V.wg_crosses_frames(4, ipf, 256)     # one workgroup per item: never
    assert max(rungs) * geom["width"] * geom["height"] * geom["channels"] <= 1400 * 9216


def test_ladder_neighbours_differ_in_every_block():
    for c in V.LADDER_CASES:
        if c.n_frames > 300:
            continue
        f = c.frames()
        sums = np.stack([V.block_sums(x, c.width, c.height, c.channels) for x in f])
        assert (sums[1:] != sums[:-1]).all()


@pytest.mark.parametrize("case", FAST, ids=_ids(FAST))
def test_numpy_bit_rule_equals_the_oracle(oracle, case):
    frames = case.frames()
    assert frames.shape == (case.n_frames, case.height, case.width * case.channels)
    assert len({f.tobytes() for f in frames[:64]}) == min(64, case.n_frames)       # distinct frames
    lits = case.claims.get("literals")
    given = case.claims["sums"](765 * case.area // 2, case.area) if case.content == "levels" else None
    for k, f in enumerate(frames):
        sums = V.block_sums(f, case.width, case.height, case.channels)
        if given is not None:
            assert (sums == given[k]).all()
        bits = V.blockhash_bits(sums, case.area)
        assert bits == oracle.blockhash(f, case.width, case.height, case.width * case.channels, case.channels), k
        if lits is not None:
            assert bits == lits[k], k


def test_finish_sizes_and_truncated_half_scale():
    assert [765 * ((w // 8) * (h // 8)) // 2 for w, h, _ in V.FINISH_SIZES] == [382, 1147, 3060]
    assert 765 * 3 % 2 == 1                                               # 1147.5: the odd area truncates
    for name, (sums, lits, kw) in V.FINISH_FRAMES.items():
        for w, h, _ in V.FINISH_SIZES:
            a = (w // 8) * (h // 8)
            for s in sums(765 * a // 2, a):
                assert len(s) == 64 and min(s) >= 0 and max(s) <= 765 * a
    c = 382
    for k in (2, 3, 4, 5):
        b = sorted(V.band_f3(k, c))
        assert b == V.band_f3(k, c) and b[16] == c and b.count(c) == k and b[14] < c < b[15 + k]
    b = V.band_f4(c)
    assert sorted(b) == b and b.count(c) == 17 and b[16] == c and b[17] > c
    b = sorted(V.band_f2(30, 600))
    assert b[15] == 30 and b[16] == 600
    assert sorted(V.PERM) == list(range(32)) and V.PERM != sorted(V.PERM)
    # F5: the two bands' medians lie on opposite sides of half scale
    for s in V._f5(c, 1):
        assert (np.sort(s[:32])[16] > c) != (np.sort(s[32:])[16] > c)
    # F7 writes alpha 0 somewhere at every size, and at areas above 1 in the frames around half scale too
    for case in V.FINISH_CASES:
        if case.claims.get("alpha0"):
            f = case.frames().reshape(case.n_frames, -1, 4)
            assert (f[-1, :, 3] == 0).all()
            if case.area > 1:
                assert all((x[:, 3] == 0).any() and (x[:, 3] == 255).any() for x in f[:3])


@pytest.mark.parametrize("case", V.ANY_SIZE_CASES, ids=_ids(V.ANY_SIZE_CASES))
def test_numpy_any_size_restatement_equals_the_oracle(oracle, case):
    assert case.stride > case.width * case.channels and case.pitch > case.stride * case.height
    frames = case.frames()
    got = [V.any_size_bits(f, case.width, case.height, case.channels) for f in frames]
    assert got == [oracle.blockhash(f, case.width, case.height, case.width * case.channels, case.channels) for f in frames]
    if case.content == "solids":
        # white: every median is above half scale and the blocks of the median's pixel count tie with it; (10, 10, 10): below, no tie bit
        px = [V.pixel_sums(f, case.width, case.height, case.channels) for f in frames]
        assert [int(p[0, 0]) for p in px] == [765, 383, 30] and all((p == p[0, 0]).all() for p in px)
        assert got[0] != got[2]      # the tie rule decides: the same ties, the median above half scale in one and below in the other


def test_the_clamp_is_needed(oracle):
    """The hard edges overshoot under Lanczos3: the resized image of the checkerboard and of the halves holds both 0 and 255, values
    the clamp made (an unclamped sum is below 0 or above 255 there, or rounds to the rail)."""
    for case in V.RESIZE_CASES:
        if (case.width, case.height) != (40, 24) or case.content not in (V.CHECKER, "halves"):
            continue
        frames = case.frames()
        for algo, _ in V.ALGOS:
            smalls = [oracle.imghash(f, case.width, case.height, case.width * case.channels, case.channels, algo)[2] for f in frames]
            assert any((s == 0).any() and (s == 255).any() for s in smalls), (case.id, algo)


def test_resize_cases_cover_the_bit_rules_ties(oracle):
    """Solid frames tie every comparison (>= mean sets all, < sets none); the sizes reach the second 256-wide block with one lane."""
    assert (257 + 255) // 256 == 2 and 257 - 256 == 1
    for case in V.RESIZE_CASES:
        assert case.stride > case.width * case.channels and case.pitch > case.stride * case.height
        if case.content != "solid":
            continue
        for f in case.frames():
            if case.channels == 4:
                assert len(set(f.reshape(-1, 4)[:, 3].tolist())) > 1 or case.width * case.height == 1     # random alpha
            assert oracle.imghash(f, case.width, case.height, case.width * case.channels, case.channels, "mean")[0] == V.ALL_ONES
            for algo in ("gradient", "vertgradient", "doublegradient"):
                assert oracle.imghash(f, case.width, case.height, case.width * case.channels, case.channels, algo)[0] == 0


def _padded(cases):
    return [c for c in cases if c.padded]


@pytest.mark.parametrize("case", _padded(BLOCKHASH), ids=_ids(_padded(BLOCKHASH)))
def test_the_poison_would_show(oracle, case):
    """Hashing the buffer as if its stride were its row length, its pitch were stride * height, or its base pointer were the
    allocation's, gives another hash: a kernel that drops one of the three does not pass on these buffers."""
    w, h, c = case.width, case.height, case.channels
    frames = case.frames()
    buf = V.pack(frames, w, h, c, case.stride, case.pitch, case.lead)
    assert buf.size == case.lead + case.pitch * case.n_frames
    body = buf[case.lead:]
    true = [oracle.blockhash(f, w, h, w * c, c) for f in frames]
    assert [oracle.blockhash(body[k * case.pitch:], w, h, case.stride, c) for k in range(case.n_frames)] == true
    n = case.n_frames       # (some frame shows it: poison is white, so a solid white frame cannot)
    if case.stride > w * c:
        assert any(oracle.blockhash(body[k * case.pitch:], w, h, w * c, c) != true[k] for k in range(n))
    if case.pitch > case.stride * h:
        assert any(oracle.blockhash(body[k * case.stride * h:], w, h, case.stride, c) != true[k] for k in range(1, n))
    if case.lead:
        assert any(oracle.blockhash(buf[k * case.pitch:], w, h, case.stride, c) != true[k] for k in range(n))
    pad = np.ones(case.pitch, bool)
    pad[: case.stride * h].reshape(h, case.stride)[:, : w * c] = False
    poison = body[: case.pitch][pad]
    if c == 4 and case.stride % 4 == 0:
        assert set(poison[3::4].tolist()) <= {0x00} and set(np.delete(poison, np.s_[3::4]).tolist()) == {0xEE}
    else:
        assert set(poison.tolist()) <= {0x00, 0xEE}


def test_resize_poison_would_show(oracle):
    for case in V.RESIZE_CASES:
        if case.content != "ramps" or case.width * case.height < 6:
            continue
        w, h, c = case.width, case.height, case.channels
        f = case.frames()[0]
        body = V.pack(case.frames(), w, h, c, case.stride, case.pitch)
        smalls = [oracle.imghash(x, w, h, s, c, "mean")[2] for x, s in ((f, w * c), (body, case.stride), (body, w * c))]
        assert (smalls[0] == smalls[1]).all() and (h == 1 or (smalls[0] != smalls[2]).any())


def test_distance_cases(oracle):
    for algo, a, b, lit in V.DISTANCE_CASES:
        if lit is not None:
            assert oracle.hash_distance(a, b) == lit
        assert oracle.hash_distance(a, b) == float(bin(a ^ b).count("1"))
    assert max(V.DISTANCE_CASES[2][1:3]) < 1 << 40


def test_group_cases_take_the_kernels_they_claim():
    for name, w, h, stride, off, k_ref, k_frame in V.GROUP_CASES:
        assert V.route(w, h, 4, stride, None, 0, 1, False) == k_ref
        assert V.route(w, h, 4, stride, None, off, 1, False) == k_frame
    assert [(c[5], c[6]) for c in V.GROUP_CASES] == [("vec", "vec"), ("vec", "bytes"), ("bytes", "bytes")]
    assert V.GROUP_CASES[0][3] > 40 * 4 and V.GROUP_CASES[0][3] % 16 == 0
