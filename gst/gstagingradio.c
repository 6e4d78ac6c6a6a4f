/* gst/gstagingradio.c — `agingradio` (GType GstRsAgingRadio), a GstAudioFilter that works in place, over the mi355fx C ABI.
 * Surface mirrored from the reference (audio/audiofx/src/agingradio/imp.rs): GType name :139-143 and agingradio/mod.rs (rank
 * NONE), six properties mutable in READY :146-197 (defaults :51-56), the white-noise-ampl rule :200-204, metadata :251-262, caps
 * F32/F64 interleaved, any rate and channel count :315-324 (allowed_caps of AudioFilterImpl), AlwaysInPlace :266-268, setup
 * :326-345 (one lowpass filter per channel), transform_ip :284-305 -> mi355_agingradio_process (the per-sample loop :94-136 runs
 * on the GPU, filter states included), stop :307-312. The reference draws from rand::rng(), seeded from the OS: a fresh seed at
 * every setup keeps the output changing from run to run. */
#include <gst/gst.h>
#include <gst/audio/audio.h>
#include <gst/audio/gstaudiofilter.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>
#include <unistd.h>
#include "../include/mi355fx.h"

GST_DEBUG_CATEGORY_STATIC(gst_rs_aging_radio_debug);
#define GST_CAT_DEFAULT gst_rs_aging_radio_debug

#define GST_TYPE_RS_AGING_RADIO (gst_rs_aging_radio_get_type())
G_DECLARE_FINAL_TYPE(GstRsAgingRadio, gst_rs_aging_radio, GST, RS_AGING_RADIO, GstAudioFilter)

struct _GstRsAgingRadio {
  GstAudioFilter parent;
  GMutex lock; /* settings */
  mi355_agingradio_settings settings;
  guint lowpass_freq;
  gboolean have_state;
  gint channels;
  gboolean f64;
  mi355_ctx *ctx;
  /* MI355_GROUP_MEMBERS=n: this process hosts n pipelines of one shape; their agingradio instances share launch sets through the
   * process-wide mi355_agroup (include/mi355fx.h: mi355_agroup_shared_agingradio) instead of a launch each */
  mi355_agroup *agroup;
  int member;
};

G_DEFINE_TYPE(GstRsAgingRadio, gst_rs_aging_radio, GST_TYPE_AUDIO_FILTER)

enum { PROP_0, PROP_WHITE_NOISE_AMPL, PROP_CLICKS_PROB, PROP_LOWPASS_FREQ, PROP_BITS_TO_QUANTIZE, PROP_CUBIC_CURVE_DISTORTION, PROP_CUBIC_CURVE_PASSES };

#define AGING_CAPS "audio/x-raw, format = (string) { " GST_AUDIO_NE(F32) ", " GST_AUDIO_NE(F64) " }, rate = (int) [ 1, MAX ], channels = (int) [ 1, MAX ], layout = (string) interleaved"

/* a new Philox key per setup from what plain C offers: the clock, the process, the instance and a counter, mixed by splitmix64 */
static guint64 aging_seed(const void *self) {
  static guint64 counter;
  struct timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  guint64 z = ((guint64)ts.tv_sec * 1000000000u + (guint64)ts.tv_nsec) ^ ((guint64)getpid() << 32) ^ (guint64)(uintptr_t)self;
  z += 0x9E3779B97F4A7C15ull * (__atomic_add_fetch(&counter, 1, __ATOMIC_RELAXED));
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void gst_rs_aging_radio_set_property(GObject *object, guint id, const GValue *value, GParamSpec *pspec) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(object);
  g_mutex_lock(&self->lock);
  switch (id) {
    case PROP_WHITE_NOISE_AMPL:
      /* changes only while there is no state (imp.rs:200-204) */
      if (!self->have_state) self->settings.white_noise_ampl = g_value_get_float(value);
      break;
    case PROP_CLICKS_PROB: self->settings.clicks_prob = g_value_get_float(value); break;
    case PROP_LOWPASS_FREQ: self->lowpass_freq = g_value_get_uint(value); break; /* takes effect at the next setup */
    case PROP_BITS_TO_QUANTIZE: self->settings.bits_to_quantize = g_value_get_float(value); break;
    case PROP_CUBIC_CURVE_DISTORTION: self->settings.cubic_curve_distortion = g_value_get_float(value); break;
    case PROP_CUBIC_CURVE_PASSES: self->settings.cubic_curve_passes = g_value_get_uint(value); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(object, id, pspec); break;
  }
  g_mutex_unlock(&self->lock);
}

static void gst_rs_aging_radio_get_property(GObject *object, guint id, GValue *value, GParamSpec *pspec) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(object);
  g_mutex_lock(&self->lock);
  switch (id) {
    case PROP_WHITE_NOISE_AMPL: g_value_set_float(value, self->settings.white_noise_ampl); break;
    case PROP_CLICKS_PROB: g_value_set_float(value, self->settings.clicks_prob); break;
    case PROP_LOWPASS_FREQ: g_value_set_uint(value, self->lowpass_freq); break;
    case PROP_BITS_TO_QUANTIZE: g_value_set_float(value, self->settings.bits_to_quantize); break;
    case PROP_CUBIC_CURVE_DISTORTION: g_value_set_float(value, self->settings.cubic_curve_distortion); break;
    case PROP_CUBIC_CURVE_PASSES: g_value_set_uint(value, self->settings.cubic_curve_passes); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(object, id, pspec); break;
  }
  g_mutex_unlock(&self->lock);
}

static gboolean gst_rs_aging_radio_start(GstBaseTransform *trans) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(trans);
  int status = 0;
  self->ctx = mi355_ctx_create(0, &status);
  if (!self->ctx) {
    GST_ELEMENT_ERROR(self, LIBRARY, INIT, ("No MI355X context"), ("%s", mi355_status_string(status)));
    return FALSE;
  }
  return TRUE;
}

/* BaseTransformImpl::stop (imp.rs:307-312): the state goes */
static gboolean gst_rs_aging_radio_stop(GstBaseTransform *trans) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(trans);
  g_mutex_lock(&self->lock);
  self->have_state = FALSE;
  g_mutex_unlock(&self->lock);
  if (self->agroup) mi355_agroup_release(self->agroup, self->member);
  self->agroup = NULL;
  if (self->ctx) mi355_ctx_destroy(self->ctx);
  self->ctx = NULL;
  return TRUE;
}

/* AudioFilterImpl::setup (imp.rs:326-345): one lowpass filter per channel when lowpass-freq > 0, a fresh state */
static gboolean gst_rs_aging_radio_setup(GstAudioFilter *filter, const GstAudioInfo *info) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(filter);
  g_mutex_lock(&self->lock);
  const guint lowpass = self->lowpass_freq;
  g_mutex_unlock(&self->lock);
  const guint channels = (guint)GST_AUDIO_INFO_CHANNELS(info), rate = (guint)GST_AUDIO_INFO_RATE(info);
  const guint64 seed = aging_seed(self);
  const char *members = g_getenv("MI355_GROUP_MEMBERS");
  if (!self->agroup && members && atoi(members) >= 2) {
    int status = 0;
    self->agroup = mi355_agroup_shared_agingradio(0, atoi(members), &self->member, &status);
    if (!self->agroup) GST_WARNING_OBJECT(self, "no shared agingradio group (%s): own launches", mi355_status_string(status));
    else (void)mi355_agroup_set_linger(self->agroup, g_getenv("MI355_GROUP_LINGER_US") ? (unsigned)atoi(g_getenv("MI355_GROUP_LINGER_US")) : 2000u, 0); /* a paused neighbour costs the others 2 ms, never a hang */
  }
  int rc = self->agroup ? mi355_agroup_agingradio_setup(self->agroup, self->member, channels, rate, lowpass, seed)
                        : mi355_agingradio_setup(self->ctx, channels, rate, lowpass, seed);
  if (rc != MI355_OK) {
    GST_ERROR_OBJECT(self, "mi355_agingradio_setup: %s", self->agroup ? mi355_agroup_last_error(self->agroup) : mi355_ctx_last_error(self->ctx));
    return FALSE;
  }
  g_mutex_lock(&self->lock);
  self->channels = (gint)channels;
  self->f64 = GST_AUDIO_INFO_FORMAT(info) == GST_AUDIO_FORMAT_F64;
  self->have_state = TRUE;
  g_mutex_unlock(&self->lock);
  return TRUE;
}

/* BaseTransformImpl::transform_ip (imp.rs:284-305): the settings are copied once per buffer */
static GstFlowReturn gst_rs_aging_radio_transform_ip(GstBaseTransform *trans, GstBuffer *buf) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(trans);
  g_mutex_lock(&self->lock);
  const mi355_agingradio_settings settings = self->settings;
  const gboolean have_state = self->have_state, f64 = self->f64;
  const gint channels = self->channels;
  g_mutex_unlock(&self->lock);
  if (!have_state) return GST_FLOW_NOT_NEGOTIATED; /* ok_or(FlowError::NotNegotiated) (imp.rs:289) */
  GstMapInfo map;
  if (!gst_buffer_map(buf, &map, GST_MAP_READWRITE)) return GST_FLOW_ERROR; /* map_writable().map_err(Error) (imp.rs:291) */
  const size_t frames = map.size / ((size_t)channels * (f64 ? sizeof(double) : sizeof(float)));
  int rc;
  if (self->agroup) { /* this buffer joins the launch set of the interval; the call returns when it has run */
    uint64_t ticket = 0;
    rc = mi355_agroup_submit_agingradio(self->agroup, self->member, map.data, frames, f64 ? 1 : 0, &settings, 0, &ticket);
    if (rc == MI355_OK) rc = mi355_agroup_wait(self->agroup, ticket, NULL);
  } else {
    rc = mi355_agingradio_process(self->ctx, map.data, frames, f64 ? 1 : 0, &settings);
  }
  gst_buffer_unmap(buf, &map);
  if (rc != MI355_OK) {
    GST_ERROR_OBJECT(self, "mi355_agingradio_process: %s", self->agroup ? mi355_agroup_last_error(self->agroup) : mi355_ctx_last_error(self->ctx));
    return GST_FLOW_ERROR;
  }
  return GST_FLOW_OK;
}

static void gst_rs_aging_radio_finalize(GObject *object) {
  GstRsAgingRadio *self = GST_RS_AGING_RADIO(object);
  g_mutex_clear(&self->lock);
  G_OBJECT_CLASS(gst_rs_aging_radio_parent_class)->finalize(object);
}

static void gst_rs_aging_radio_class_init(GstRsAgingRadioClass *klass) {
  GObjectClass *gobject = G_OBJECT_CLASS(klass);
  GstElementClass *element = GST_ELEMENT_CLASS(klass);
  GstBaseTransformClass *trans = GST_BASE_TRANSFORM_CLASS(klass);
  GstAudioFilterClass *afilter = GST_AUDIO_FILTER_CLASS(klass);
  gobject->set_property = gst_rs_aging_radio_set_property;
  gobject->get_property = gst_rs_aging_radio_get_property;
  gobject->finalize = gst_rs_aging_radio_finalize;
  const GParamFlags f = (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS | GST_PARAM_MUTABLE_READY);
  g_object_class_install_property(gobject, PROP_WHITE_NOISE_AMPL,
      g_param_spec_float("white-noise-ampl", "White noise amplitude", "White noise amplitude (0 to disable)", 0.0f, 1.0f, 0.011f, f));
  g_object_class_install_property(gobject, PROP_CLICKS_PROB,
      g_param_spec_float("clicks-prob", "Clicks probability", "Clicks probability (0 to disable)", 0.0f, 1.0f, 1.0f / 100000.0f, f));
  g_object_class_install_property(gobject, PROP_LOWPASS_FREQ,
      g_param_spec_uint("lowpass-freq", "Lowpass filter frequency", "Lowpass filter frequency (0 to disable)", 0, 22000, 2000, f));
  g_object_class_install_property(gobject, PROP_BITS_TO_QUANTIZE,
      g_param_spec_float("bits-to-quantize", "Bits to quantize", "Bits to quantize (0 to disable)", 0.0f, 64.0f, 4.0f, f));
  g_object_class_install_property(gobject, PROP_CUBIC_CURVE_DISTORTION,
      g_param_spec_float("cubic-curve-distortion", "Cubic curve distortion", "Cubic curve distortion (0 to disable)", 0.0f, 1.0f, 1.0f, f));
  g_object_class_install_property(gobject, PROP_CUBIC_CURVE_PASSES,
      g_param_spec_uint("cubic-curve-passes", "Cubic curve passes", "Cubic curve passes (0 to disable)", 0, G_MAXUINT, 3, f));
  gst_element_class_set_static_metadata(element, "Aging Radio", "Filter/Effect/Audio", "Adds age to audio input using various kinds of distortion",
                                        "Vivia Nikolaidou <vivia@ahiru.eu>");
  GstCaps *caps = gst_caps_from_string(AGING_CAPS);
  gst_audio_filter_class_add_pad_templates(afilter, caps); /* AudioFilterImpl::allowed_caps (imp.rs:315-324) */
  gst_caps_unref(caps);
  trans->start = gst_rs_aging_radio_start;
  trans->stop = gst_rs_aging_radio_stop;
  trans->transform_ip = gst_rs_aging_radio_transform_ip; /* only _ip installed == BaseTransformMode::AlwaysInPlace (imp.rs:266) */
  trans->passthrough_on_same_caps = FALSE;
  trans->transform_ip_on_passthrough = FALSE;
  afilter->setup = gst_rs_aging_radio_setup;
  GST_DEBUG_CATEGORY_INIT(gst_rs_aging_radio_debug, "agingradio", 0, "Rust Aging Radio Filter (MI355X)");
}

static void gst_rs_aging_radio_init(GstRsAgingRadio *self) {
  g_mutex_init(&self->lock);
  self->settings.white_noise_ampl = 0.011f;          /* DEFAULT_WHITE_NOISE_AMPL (imp.rs:51) */
  self->settings.clicks_prob = 1.0f / 100000.0f;     /* DEFAULT_CLICKS_PROB (imp.rs:52) */
  self->lowpass_freq = 2000;                         /* DEFAULT_LOWPASS_FREQ (imp.rs:53) */
  self->settings.bits_to_quantize = 4.0f;            /* DEFAULT_BITS_TO_QUANTIZE (imp.rs:54) */
  self->settings.cubic_curve_distortion = 1.0f;      /* DEFAULT_CUBIC_CURVE_DISTORTION (imp.rs:55) */
  self->settings.cubic_curve_passes = 3;             /* DEFAULT_CUBIC_CURVE_PASSES (imp.rs:56) */
}

gboolean gst_rs_aging_radio_register(GstPlugin *plugin) {
  return gst_element_register(plugin, "agingradio", GST_RANK_NONE, GST_TYPE_RS_AGING_RADIO); /* agingradio/mod.rs */
}
