"""agingradio without a GPU: the restatement of DESIGN §4.9 (Philox known answers, hand-worked values, the distributions of the
draws) and the GStreamer shim's surface against tests/golden/agingradio_surface.json (from docs/plugins/gst_plugins_cache.json)."""
import json
import math
import os
import re
import subprocess

import numpy as np

import agingradio_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GST = os.path.join(ROOT, "gst")
SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "agingradio_surface.json")))["agingradio"]


def _words(*a):
    return tuple(int(v) for v in R.philox4x32_10(*a))


def test_philox_known_answers():
    assert _words(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    m = 0xFFFFFFFF
    assert _words(m, m, m, m, m, m) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert _words(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_draw_slots_pick_the_64_bit_words():
    seed = 0x0123456789ABCDEF
    pairs = np.array([0, 1, 1 << 40], np.uint64)
    x0, x1, x2, x3 = R.philox4x32_10(pairs & np.uint64(0xFFFFFFFF), pairs >> np.uint64(32), 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    assert np.array_equal(R.draws(pairs, 0, seed), (x1 << np.uint64(32)) | x0)
    assert np.array_equal(R.draws(pairs, 1, seed), (x3 << np.uint64(32)) | x2)
    y0 = R.philox4x32_10(pairs & np.uint64(0xFFFFFFFF), pairs >> np.uint64(32), 1, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    assert np.array_equal(R.draws(pairs, 2, seed) & np.uint64(0xFFFFFFFF), y0)


def _run(data, channels=1, rate=48000, seed=7, **settings):
    s = dict(R.OFF, **settings)
    a = R.AgingRadio(channels, rate, s["lowpass_freq"], seed)
    return a.process(np.asarray(data), **s), a


def test_everything_disabled_is_the_identity():
    rng = np.random.default_rng(1)
    for dt in (np.float32, np.float64):
        x = (rng.standard_normal(2 * 101) * 3).astype(dt)
        y, _ = _run(x, channels=2)
        assert y.dtype == dt and y.tobytes() == x.tobytes()


def test_odd_frame_count_leaves_the_last_frame_untouched():
    x = np.full(3 * 5, 0.3)
    y, a = _run(x, channels=3, bits_to_quantize=1.0, clicks_prob=1.0)
    assert np.all(y[:12] == 1.0) and np.array_equal(y[12:], x[12:]) and a.k == 2


def test_quantise_rounds_half_away_from_zero():
    y, _ = _run([0.03125, -0.03125, 0.09375, 0.0], bits_to_quantize=4.0)
    assert y.tolist() == [0.0625, -0.0625, 0.125, 0.0]


def test_cubic_curve_passes():
    for passes, want in ((1, 0.375), (2, 0.322265625), (3, 38761635 / 2 ** 27)):
        y, _ = _run([0.5, 0.5], cubic_curve_distortion=1.0, cubic_curve_passes=passes)
        assert y[0] == want, passes
    y, _ = _run(np.array([0.5, 0.5], np.float32), cubic_curve_distortion=1.0, cubic_curve_passes=3)
    assert float(y[0]) == 38761636 / 2 ** 27


def test_lowpass_coefficient_and_step_response():
    alpha = R.lowpass_alpha(48000, 2000)
    assert alpha == 0.20748099129750258
    y, a = _run(np.ones(64), lowpass_freq=2000)
    prev = 0.0
    for n in range(64):
        prev = prev + alpha * (1.0 - prev)
        assert y[n] == prev, n
    assert a.y[0] == prev


def test_certain_clicks_set_every_pair_and_freeze_the_filter():
    y, a = _run(np.linspace(-0.5, 0.5, 2 * 40), channels=2, lowpass_freq=2000, clicks_prob=1.0, white_noise_ampl=0.5, bits_to_quantize=3.0)
    assert np.all(y == 1.0) and np.all(a.y == 0.0) and a.k == 20
    assert R.p_int(1.0) == R.ALWAYS and R.p_int(0.5) == 1 << 63


def test_nan_stays_nan_and_inf_is_clamped_before_the_filter():
    y, _ = _run([math.nan, 0.25], bits_to_quantize=4.0, cubic_curve_distortion=0.5, cubic_curve_passes=2, lowpass_freq=2000)
    assert math.isnan(y[0]) and math.isnan(y[1])
    alpha = R.lowpass_alpha(48000, 2000)
    y, a = _run([math.inf, -math.inf], lowpass_freq=2000)
    y1 = alpha * 1.0
    assert y[0] == y1 and y[1] == y1 + alpha * (-1.0 - y1) and a.y[0] == y[1]
    y, _ = _run([math.inf, -math.inf])   # no lowpass: no clamp
    assert y[0] == math.inf and y[1] == -math.inf


def test_noise_distribution():
    a = float(np.float32(0.011))
    n = R.noise(R.draws(np.arange(1 << 20, dtype=np.uint64), 3, 99), a)
    assert np.all(n >= -a) and np.all(n < a)
    assert abs(n.mean()) < 6 * a / math.sqrt(3 * n.size)          # uniform: sigma = a / sqrt(3)
    assert abs(n.var() - a * a / 3) < 0.01 * a * a
    # the largest draw stays below a for many f32 amplitudes (no rejection step needed)
    top = ((np.uint64((1 << 52) - 1)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0
    amps = np.random.default_rng(3).random(200000).astype(np.float32).astype(np.float64)
    amps = amps[amps > 0]
    assert np.all(top * (amps + amps) + (-amps) < amps)


def test_click_frequency_is_binomial():
    p = float(np.float32(0.01))
    N = 1 << 20
    k = int(np.count_nonzero(R.draws(np.arange(N, dtype=np.uint64), 0, 12345) < np.uint64(R.p_int(p))))
    sd = math.sqrt(N * p * (1 - p))
    assert abs(k - N * p) < 6 * sd


def test_state_carries_over_ragged_buffers():
    rng = np.random.default_rng(2)
    s = dict(R.DEFAULTS, clicks_prob=0.05)
    x = rng.uniform(-1, 1, 3 * 400)
    whole = R.AgingRadio(3, 44100, 2000, 5).process(x, **s)
    a = R.AgingRadio(3, 44100, 2000, 5)
    out, pos = [], 0
    for n in (2, 10, 64, 124, 200):   # even frame counts: an odd one drops a frame from the pair walk
        out.append(a.process(x[pos:pos + 3 * n], **s))
        pos += 3 * n
    assert np.array_equal(np.concatenate(out), whole)


def test_shim_carries_the_pinned_surface():
    src = open(os.path.join(GST, "gstagingradio.c")).read()
    assert re.search(r'gst_element_register\(plugin, "agingradio", GST_RANK_NONE, GST_TYPE_RS_AGING_RADIO\)', src) and SURFACE["rank"] == "none"
    assert "G_DEFINE_TYPE(%s, gst_rs_aging_radio, GST_TYPE_AUDIO_FILTER)" % SURFACE["type_name"] in src and SURFACE["parent"] == "GstAudioFilter"
    assert 'gst_element_class_set_static_metadata(element, "%s", "%s", "%s",' % (SURFACE["long_name"], SURFACE["klass"], SURFACE["description"]) in src
    assert '"%s"' % SURFACE["author"] in src
    for name, p in SURFACE["properties"].items():
        assert p["mutable"] == "ready"
        if p["type"] == "gfloat":
            want = r'g_param_spec_float\("%s", "[^"]*", "%s", %sf, %sf, [^,]+, f\)' % (name, re.escape(p["blurb"]), float(p["min"]), float(p["max"]))
            m = re.search(want, src)
            assert m, name
            default = re.search(r'g_param_spec_float\("%s",[^;]*, ([^,]+), f\)' % name, src).group(1)
            assert np.float32(eval(default.replace("f", ""))) == np.float32(float(p["default"])), name
        else:
            assert p["type"] == "guint"
            hi = "G_MAXUINT" if p["max"] == "-1" else p["max"]
            assert re.search(r'g_param_spec_uint\("%s", "[^"]*", "%s", %s, %s, %s, f\)' % (name, re.escape(p["blurb"]), p["min"], hi, p["default"]), src), name
    assert "GST_PARAM_MUTABLE_READY" in src
    for caps in (SURFACE["caps"], SURFACE["src_caps"]):
        assert "rate: [ 1, 2147483647 ]" in caps and "channels: [ 1, 2147483647 ]" in caps and "layout: interleaved" in caps and "{ F32LE, F64LE }" in caps
    assert 'GST_AUDIO_NE(F32) ", " GST_AUDIO_NE(F64)' in src and "rate = (int) [ 1, MAX ], channels = (int) [ 1, MAX ], layout = (string) interleaved" in src
    assert "trans->transform_ip = gst_rs_aging_radio_transform_ip;" in src and "afilter->setup = gst_rs_aging_radio_setup;" in src
    assert "trans->transform =" not in src and "trans->passthrough_on_same_caps = FALSE;" in src
    assert "mi355_agingradio_setup(" in src and "mi355_agingradio_process(" in src and "mi355_agroup_shared_agingradio(" in src
    assert "mi355_agroup_submit_agingradio(" in src and "g_random" not in src
    assert "if (!self->have_state) self->settings.white_noise_ampl" in src
    plugin = open(os.path.join(GST, "plugin_rsaudiofx.c")).read()
    order = [plugin.index("gst_%s_register(plugin)" % n) for n in ("rs_aging_radio", "rs_audio_echo", "audio_loud_norm", "ebur128_level")]
    assert order == sorted(order) and SURFACE["registered_before"] == "rsaudioecho"
    assert "audiornnoise" in plugin and "stay with the reference" not in plugin
    mk = open(os.path.join(GST, "Makefile")).read()
    assert "gstagingradio.c" in re.search(r"^libgstrsaudiofx\.so:.*$", mk, flags=re.M).group(0)


def test_shim_syntax_covers_the_new_file():
    r = subprocess.run(["make", "-C", GST, "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len([f for f in os.listdir(GST) if f.endswith(".c")])
    assert os.path.exists(os.path.join(GST, "gstagingradio.c")) and "syntax ok: %d files" % n in r.stdout


def test_host_element_carries_the_surface():
    from mi355fx.elements import _lib
    import ctypes as C
    L = _lib()
    err = C.create_string_buffer(256)
    h = L.mi355el_agingradio_new(0, err, 256)
    if not h:   # no device here: the element needs its context (no CPU fallback); the error says so
        assert b"device context" in err.value, err.value
        return
    try:
        assert L.mi355el_type_name(h).decode() == SURFACE["type_name"] and L.mi355el_klass(h).decode() == SURFACE["klass"]
    finally:
        L.mi355el_free(h)


def test_library_exports_the_entry_points(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    for name in ("mi355_agingradio_setup", "mi355_agingradio_process", "mi355_agingradio_process_device", "mi355_agingradio_get_state",
                 "mi355_agingradio_reset", "mi355_agroup_create_agingradio", "mi355_agroup_shared_agingradio", "mi355_agroup_agingradio_setup",
                 "mi355_agroup_submit_agingradio", "mi355_agroup_agingradio_get_state"):
        assert name + "(" in hdr and hasattr(mi355lib, name) and getattr(mi355lib, name).argtypes is not None

