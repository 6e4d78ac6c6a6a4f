"""GPU tests of the exact Dssim engine's kernels branch by branch: every case of tests/dssim_cases.py (proved on the CPU by
test_dssim_cases_cpu.py) goes through every route - host and device create_image, the two-step compare with its insides
(mi355_selftest_dssim_compare_detail), compare_frames, the pairs entry and the pair-map diagnostic at MI355_FLAG_DSSIM_FAST = 0 -
against the numpy restatement (oracle/dssim_restate.py): planes and SSIM maps bit for bit, the f64 reduction slots within the bound
of an n-term sum in any order, the value within the suite's rel 1e-9 / abs 1e-13."""
import math

import numpy as np
import pytest

import dssim_cases as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
IDS = [g.id for g in T.GEOMETRIES]


def _upload(ctx, buf):
    d = ctx.alloc(buf.nbytes)
    assert d % 8 == 0
    ctx.h2d(d, buf)
    return d


def _set_pattern(ctx, case):
    import mi355fx
    ctx.set_flag(mi355fx.FLAG_DSSIM_TRANSLUCENT, 0 if case.pattern else 1)


def _bits_equal(got, exp):
    return got.shape == exp.shape and bool((got.view(np.uint32) == exp.view(np.uint32)).all())


def _planes_are(ctx, img, oracle_image, what):
    for s, chans in enumerate(oracle_image.scales):
        for ch in range(3):
            for kind in ("img", "mu", "sq"):
                got = ctx.dssim_image_plane(img, s, ch, kind)
                assert _bits_equal(got, chans[ch][kind]), (what, s, ch, kind, int((got != chans[ch][kind]).sum()))


@pytest.mark.parametrize("g", T.GEOMETRIES, ids=IDS)
def test_create_image_planes_are_the_restatements_through_the_host_and_the_device_entry(ctx, g):
    """All nine planes of every scale of both frames of every case, bit for bit: scale kernel (interior and border path, grouped
    launches), both downsample kernels and the byte-load form the case's layout selects."""
    import mi355fx
    try:
        for c in g.cases:
            _set_pattern(ctx, c)
            _, _, oa, ob = T.reference(c)
            for buf, o, which in zip(c.buffers(), (oa, ob), ("ref", "mod")):
                host = ctx.dssim_create_image(buf[c.lead:], c.stride, c.w, c.h, c.fmt)
                d = _upload(ctx, buf)
                try:
                    assert T.u8_form(c.channels, d + c.lead, c.stride) == c.device_form()
                    dev = ctx.dssim_create_image_device(d + c.lead, c.stride, c.w, c.h, c.fmt)
                    try:
                        _planes_are(ctx, host, o, (c.id, which, "host"))
                        _planes_are(ctx, dev, o, (c.id, which, "device"))
                    finally:
                        ctx.dssim_free_image(dev)
                finally:
                    ctx.dssim_free_image(host)
                    ctx.synchronize()
                    ctx.free(d)
    finally:
        ctx.set_flag(mi355fx.FLAG_DSSIM_TRANSLUCENT, 0)


def _check_slots(case, k, m, slots):
    """The [sum, avg, dev] slots of scale k against the map the device itself wrote (m, already held to the restatement bit for bit).
    Returns the distance of avg from numpy's power in ulps."""
    mm = m.astype(np.float64).reshape(-1)
    n = mm.size
    s_exact = math.fsum(mm)
    assert abs(slots[0] - s_exact) <= (n - 1) * U * math.fsum(np.abs(mm)), (case.id, k, slots[0], s_exact)
    ulps = 0.0
    if s_exact < 0.0:
        assert slots[1] == 0.0, (case.id, k, slots[1])                      # the clamp on a negative mean
    else:
        exp = float(np.power(np.float64(max(slots[0] / n, 0.0)), np.float64(0.5 ** k)))
        ulps = abs(slots[1] - exp) / float(np.spacing(np.float64(exp)))
        assert abs(slots[1] - exp) <= 1e-12 * abs(exp), (case.id, k, slots[1], exp)
    dev = np.abs(slots[1] - mm)
    d_exact = math.fsum(dev)
    assert abs(slots[2] - d_exact) <= (n + 1) * U * d_exact, (case.id, k, slots[2], d_exact)
    return ulps


@pytest.mark.parametrize("g", T.GEOMETRIES, ids=IDS)
def test_two_step_compare_maps_slots_and_value(ctx, g):
    """dssim_compare_fused_kernel and the three reduction kernels: every scale's SSIM map bit for bit, every slot within its bound,
    avg exactly 0.0 where the mean SSIM is negative, the value within rel 1e-9 / abs 1e-13; identical frames give exactly 0.0 and
    maps of all 1.0."""
    import mi355fx
    worst = 0.0
    try:
        for c in g.cases:
            negative = []
            _set_pattern(ctx, c)
            exp, maps, _, _ = T.reference(c)
            ref, mod = c.buffers()
            a = ctx.dssim_create_image(ref[c.lead:], c.stride, c.w, c.h, c.fmt)
            b = ctx.dssim_create_image(mod[c.lead:], c.stride, c.w, c.h, c.fmt)
            try:
                value = ctx.dssim_compare(a, b)
                for k, m_exp in enumerate(maps):
                    v, m, slots = ctx.selftest_dssim_compare_detail(a, b, k)
                    assert v == value
                    assert _bits_equal(m, m_exp), (c.id, k, int((m != m_exp).sum()))
                    worst = max(worst, _check_slots(c, k, m, slots))
                    if slots[1] == 0.0:
                        negative.append(k)
                    if c.content == "identical":
                        assert (m == 1.0).all() and slots == [float(m.size), 1.0, 0.0], (c.id, k, slots)
                with pytest.raises(mi355fx.Mi355Error):
                    ctx.selftest_dssim_compare_detail(a, b, len(maps))
                assert value == pytest.approx(exp, rel=1e-9, abs=1e-13), (c.id, value, exp)
                if c.content == "identical":
                    assert value == 0.0
                if c.content == "inverted":
                    assert tuple(negative) == T.NEGATIVE_MEAN[g.id]
            finally:
                ctx.dssim_free_image(a)
                ctx.dssim_free_image(b)
        print("dssim routes %s: avg is at most %.2f ulp from numpy's power of the device's sum" % (g.id, worst))
    finally:
        ctx.set_flag(mi355fx.FLAG_DSSIM_TRANSLUCENT, 0)


def _pair_map(ctx, da, db, c, k, mw, mh):
    """The SSIM map of scale k through a NaN-filled buffer: all of the map is written, nothing behind it."""
    buf = np.full(mw * mh + 64, np.nan, np.float32)
    ctx.dssim_pair_map_device(da, db, c.stride, c.w, c.h, c.fmt, k, buf)
    assert np.isnan(buf[mw * mh:]).all(), "written past the map"
    assert np.isfinite(buf[:mw * mh]).all(), "map pixels left unwritten"
    return buf[:mw * mh].reshape(mh, mw)


@pytest.mark.parametrize("g", T.GEOMETRIES, ids=IDS)
def test_compare_frames_pairs_and_pair_maps(ctx, g):
    """dssim_hash_compare_kernel (interior and border path, grouped launches, several frames per reduction launch). All the cases of
    a geometry that one call can take - one byte layout, one setting of the translucency flag - go through compare_frames in ONE
    call against the first case's reference image, host and device, == the two-step values of the same frames; every case's own
    (reference, modified) pair goes through the pairs entry, all in one call, == compare_frames of that pair, within rel 1e-9 /
    abs 1e-13 of the restatement; the pair-map diagnostic returns every scale's map of every case bit for bit."""
    import mi355fx
    ctx.set_flag(mi355fx.FLAG_DSSIM_FAST, 0)
    try:
        for group in g.groups():
            c0 = group[0]
            lead, geom = c0.lead, (c0.stride, c0.w, c0.h, c0.fmt)
            _set_pattern(ctx, c0)
            refs = [c.buffers()[0] for c in group]
            mods = [c.buffers()[1] for c in group]
            a = ctx.dssim_create_image(refs[0][lead:], *geom)
            bufs = []
            try:
                two_step = []
                for m in mods:
                    b = ctx.dssim_create_image(m[lead:], *geom)
                    two_step.append(ctx.dssim_compare(a, b))
                    ctx.dssim_free_image(b)
                fused = ctx.dssim_compare_frames(a, [m[lead:] for m in mods], *geom)
                assert fused == two_step, (c0.id, fused, two_step)
                d_refs, d_mods = [], []
                for r, m in zip(refs, mods):
                    d_refs.append(_upload(ctx, r) + lead)
                    d_mods.append(_upload(ctx, m) + lead)
                    bufs += [d_refs[-1] - lead, d_mods[-1] - lead]
                assert ctx.dssim_compare_frames_device(a, d_mods, *geom) == fused
                # every case's own pair: compare_frames against its own reference image, then all pairs in one call
                own = []
                for c, r, dm, f in zip(group, refs, d_mods, fused):
                    if c.ref_key == c0.ref_key:
                        assert (r == refs[0]).all()
                        own.append(f)
                    else:
                        x = ctx.dssim_create_image(r[lead:], *geom)
                        own.append(ctx.dssim_compare_frames_device(x, [dm], *geom)[0])
                        ctx.dssim_free_image(x)
                pairs = ctx.dssim_compare_pairs_device(d_refs, d_mods, *geom)
                assert pairs == own, (c0.id, pairs, own)
                for c, dr, dm, v in zip(group, d_refs, d_mods, own):
                    exp, maps, _, _ = T.reference(c)
                    assert v == pytest.approx(exp, rel=1e-9, abs=1e-13), (c.id, v, exp)
                    if c.content == "identical":
                        assert v == 0.0
                    for k, m_exp in enumerate(maps):
                        m = _pair_map(ctx, dr, dm, c, k, m_exp.shape[1], m_exp.shape[0])
                        assert _bits_equal(m, m_exp), (c.id, k, int((m != m_exp).sum()))
                        if c.content == "identical":
                            assert (m == 1.0).all()
            finally:
                ctx.dssim_free_image(a)
                ctx.synchronize()
                for d in bufs:
                    ctx.free(d)
    finally:
        ctx.set_flag(mi355fx.FLAG_DSSIM_TRANSLUCENT, 0)
