/* gst/gstcolordetect.c — `colordetect` (GType GstColorDetect), a GstVideoFilter that reads every frame in place and never writes
 * it, over the mi355fx C ABI. Surface mirrored from the reference (video/videofx/src/colordetect/imp.rs): GType name :116-121
 * and colordetect/mod.rs (rank NONE), properties quality (guint 0..10, default 10) and max-colors (guint 2..255, default 2), both
 * mutable in PLAYING :123-148 (defaults :19-20), metadata :202-215, sink / src {RGB, RGBA, ARGB, BGR, BGRA} :217-245,
 * AlwaysInPlace + passthrough on same caps + transform_ip on passthrough :247-250, stop drops the state :252-256, set_info keeps
 * the colour posted last :260-294, transform_frame_ip_passthrough :296-307 -> detect_color :57-84 (get_palette of plane_data(0)
 * runs on the GPU: mi355_colordetect_frame) and color_changed :86-113 (one "colordetect" element message per change of the
 * dominant colour's css name).
 * A buffer of our device memory (gst_mi355_buffer_peek_device) is read where it lies: mi355_colordetect_frames_device on its
 * device pointer, only the palette comes back. With MI355_GROUP_MEMBERS=n (n >= 2) in the environment the n
 * instances of the process hand those device frames to the device's dispatcher instead (mi355_group_submit_colordetect): the
 * frames of an interval share one histogram launch, one MMCQ launch and one copy. */
#include <stdlib.h>
#include <string.h>

#include "../gst-plugins-rs_amd/host/mi355fx_host.h"
#include "gstmi355common.h"

#ifndef G_TYPE_UINT
#define G_TYPE_UINT ((GType)(7 << 2)) /* G_TYPE_MAKE_FUNDAMENTAL (7): for the declaration-only build of `make syntax` */
#endif

GST_DEBUG_CATEGORY_STATIC(gst_color_detect_debug);
#define GST_CAT_DEFAULT gst_color_detect_debug

#define GST_TYPE_COLOR_DETECT (gst_color_detect_get_type())
G_DECLARE_FINAL_TYPE(GstColorDetect, gst_color_detect, GST, COLOR_DETECT, GstVideoFilter)

struct _GstColorDetect {
  GstVideoFilter parent;
  GMutex lock; /* settings: set from application threads, snapshotted once per frame (imp.rs:68) */
  guint quality, max_colors;
  /* state (imp.rs:45-48): present between set_info and stop; the streaming thread only */
  gboolean have_state;
  int format;
  gchar *current_color;
  mi355_ctx *ctx;
  /* MI355_GROUP_MEMBERS=n: the process's dispatcher (mi355_group_shared), held between start and stop */
  mi355_group *group;
};

G_DEFINE_TYPE(GstColorDetect, gst_color_detect, GST_TYPE_VIDEO_FILTER)

enum { PROP_0, PROP_QUALITY, PROP_MAX_COLORS };

#define CD_FORMATS "{ RGB, RGBA, ARGB, BGR, BGRA }"
static GstStaticPadTemplate sink_template =
    GST_STATIC_PAD_TEMPLATE("sink", GST_PAD_SINK, GST_PAD_ALWAYS, GST_STATIC_CAPS(GST_VIDEO_CAPS_MAKE(CD_FORMATS)));
static GstStaticPadTemplate src_template =
    GST_STATIC_PAD_TEMPLATE("src", GST_PAD_SRC, GST_PAD_ALWAYS, GST_STATIC_CAPS(GST_VIDEO_CAPS_MAKE(CD_FORMATS)));

static void gst_color_detect_set_property(GObject *object, guint id, const GValue *value, GParamSpec *pspec) {
  GstColorDetect *self = GST_COLOR_DETECT(object);
  g_mutex_lock(&self->lock);
  switch (id) {
    case PROP_QUALITY: self->quality = g_value_get_uint(value); break;
    case PROP_MAX_COLORS: self->max_colors = g_value_get_uint(value); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(object, id, pspec); break;
  }
  g_mutex_unlock(&self->lock);
}

static void gst_color_detect_get_property(GObject *object, guint id, GValue *value, GParamSpec *pspec) {
  GstColorDetect *self = GST_COLOR_DETECT(object);
  g_mutex_lock(&self->lock);
  switch (id) {
    case PROP_QUALITY: g_value_set_uint(value, self->quality); break;
    case PROP_MAX_COLORS: g_value_set_uint(value, self->max_colors); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(object, id, pspec); break;
  }
  g_mutex_unlock(&self->lock);
}

static gboolean gst_color_detect_start(GstBaseTransform *trans) {
  GstColorDetect *self = GST_COLOR_DETECT(trans);
  int status = 0;
  self->ctx = mi355_ctx_create(0, &status);
  if (!self->ctx) {
    GST_ELEMENT_ERROR(self, LIBRARY, INIT, ("No MI355X context"), ("%s", mi355_status_string(status)));
    return FALSE;
  }
  const char *members = g_getenv("MI355_GROUP_MEMBERS");
  if (members && atoi(members) >= 2 && (self->group = mi355_group_shared(0, &status)))
    (void)mi355_group_set_colordetect_rendezvous(self->group, atoi(members), 2000); /* every instance submits + waits at once; a straggler is waited for 2 ms */
  return TRUE;
}

/* BaseTransformImpl::stop (imp.rs:252-256): the state goes, with it the colour posted last */
static gboolean gst_color_detect_stop(GstBaseTransform *trans) {
  GstColorDetect *self = GST_COLOR_DETECT(trans);
  self->have_state = FALSE;
  g_free(self->current_color);
  self->current_color = NULL;
  if (self->group) mi355_group_release(self->group);
  self->group = NULL;
  if (self->ctx) mi355_ctx_destroy(self->ctx);
  self->ctx = NULL;
  GST_INFO_OBJECT(self, "Stopped");
  return TRUE;
}

/* VideoFilterImpl::set_info (imp.rs:260-294): a new state for the format; current_color carries over */
static gboolean gst_color_detect_set_info(GstVideoFilter *filter, GstCaps *incaps, GstVideoInfo *in_info, GstCaps *outcaps, GstVideoInfo *out_info) {
  GstColorDetect *self = GST_COLOR_DETECT(filter);
  const GstVideoFormat f = GST_VIDEO_INFO_FORMAT(in_info);
  if (f != GST_VIDEO_FORMAT_RGB && f != GST_VIDEO_FORMAT_RGBA && f != GST_VIDEO_FORMAT_ARGB && f != GST_VIDEO_FORMAT_BGR && f != GST_VIDEO_FORMAT_BGRA)
    return FALSE;
  self->format = gst_mi355_format(f);
  self->have_state = TRUE;
  GST_DEBUG_OBJECT(self, "Configured for format %d", self->format);
  return TRUE;
}

/* color_changed (imp.rs:86-113): "dominant-color" and "palette", a list of guint (r << 16) | (g << 8) | b in palette order */
static void gst_color_detect_post(GstColorDetect *self, const gchar *name, const uint8_t *rgb, int n) {
  GValue list = G_VALUE_INIT;
  g_value_init(&list, GST_TYPE_LIST);
  for (int k = 0; k < n; k++) {
    GValue v = G_VALUE_INIT;
    g_value_init(&v, G_TYPE_UINT);
    g_value_set_uint(&v, ((guint)rgb[3 * k] << 16) | ((guint)rgb[3 * k + 1] << 8) | (guint)rgb[3 * k + 2]);
    gst_value_list_append_and_take_value(&list, &v);
  }
  GstStructure *s = gst_structure_new("colordetect", "dominant-color", G_TYPE_STRING, name, NULL);
  gst_structure_take_value(s, "palette", &list);
  GST_DEBUG_OBJECT(self, "Dominant color changed to %s", name);
  (void)gst_element_post_message(GST_ELEMENT(self), gst_message_new_element(GST_OBJECT(self), s));
}

/* detect_color (imp.rs:57-84) on a host plane (d_frames == NULL) or a device one */
static GstFlowReturn gst_color_detect_detect(GstColorDetect *self, const uint8_t *data, const uint8_t *d_data, size_t size) {
  if (!self->have_state) {
    GST_ELEMENT_ERROR(self, CORE, NEGOTIATION, ("Have no state yet"), (NULL));
    return GST_FLOW_NOT_NEGOTIATED;
  }
  guint quality, max_colors;
  g_mutex_lock(&self->lock);
  quality = self->quality;
  max_colors = self->max_colors;
  g_mutex_unlock(&self->lock);
  uint8_t rgb[255 * 3];
  int n = 0;
  int rc;
  const gboolean grouped = d_data && self->group;
  if (grouped) { /* the frame joins whatever the other instances have pending; the palette is the lone call's, byte for byte */
    uint64_t ticket = 0;
    rc = mi355_group_submit_colordetect(self->group, self->ctx, d_data, size, self->format, (int)quality, (int)max_colors, &ticket);
    if (rc == MI355_OK) rc = mi355_group_wait_colordetect(self->group, ticket, rgb, &n);
  } else {
    rc = d_data ? mi355_colordetect_frames_device(self->ctx, d_data, size, size, 1, self->format, (int)quality, (int)max_colors, rgb, &n)
                : mi355_colordetect_frame(self->ctx, data, size, self->format, (int)quality, (int)max_colors, rgb, &n);
  }
  if (rc != MI355_OK || n == 0) { /* get_palette's Err -> FlowError::Error; no colour: the reference fails at palette[0] */
    GST_ERROR_OBJECT(self, "colordetect: %s",
                     rc == MI355_OK ? "no colour in the frame" : (grouped ? mi355_group_last_error(self->group) : mi355_ctx_last_error(self->ctx)));
    return GST_FLOW_ERROR;
  }
  const gchar *name = mi355host_css_color_similar(rgb[0], rgb[1], rgb[2]);
  if (self->current_color && strcmp(self->current_color, name) == 0) return GST_FLOW_OK;
  g_free(self->current_color);
  self->current_color = g_strdup(name);
  gst_color_detect_post(self, name, rgb, n);
  return GST_FLOW_OK;
}

/* GstBaseTransformClass::transform_ip, in front of GstVideoFilter's (which maps the buffer): a buffer of our device memory is read
 * where it lies - only the palette crosses PCIe; anything else chains up to transform_frame_ip below. */
static GstFlowReturn gst_color_detect_transform_ip(GstBaseTransform *trans, GstBuffer *buf) {
  GstColorDetect *self = GST_COLOR_DETECT(trans);
  GstVideoFilter *vf = GST_VIDEO_FILTER(trans);
  mi355_buf *b = gst_mi355_buffer_peek_device(buf);
  if (!b || !vf->negotiated || !self->have_state) return GST_BASE_TRANSFORM_CLASS(gst_color_detect_parent_class)->transform_ip(trans, buf);
  const GstVideoInfo *ii = &vf->in_info;
  /* plane_data(0) is stride x height bytes at the plane's offset (gstreamer-rs VideoFrame::plane_data) */
  const size_t offset = GST_VIDEO_INFO_PLANE_OFFSET(ii, 0), size = (size_t)GST_VIDEO_INFO_PLANE_STRIDE(ii, 0) * (size_t)GST_VIDEO_INFO_HEIGHT(ii);
  const uint8_t *d = mi355_buf_device_ptr(b, self->ctx, MI355_MAP_READ);
  if (!d) {
    GST_ERROR_OBJECT(self, "mi355_buf_device_ptr: %s", mi355_ctx_last_error(self->ctx));
    return GST_FLOW_ERROR;
  }
  return gst_color_detect_detect(self, NULL, d + offset, size);
}

/* transform_frame_ip_passthrough (imp.rs:296-307): the frame is mapped READ by the parent class in passthrough */
static GstFlowReturn gst_color_detect_transform_frame_ip(GstVideoFilter *filter, GstVideoFrame *frame) {
  GstColorDetect *self = GST_COLOR_DETECT(filter);
  const size_t size = (size_t)GST_VIDEO_FRAME_PLANE_STRIDE(frame, 0) * (size_t)GST_VIDEO_FRAME_HEIGHT(frame); /* plane_data(0) */
  return gst_color_detect_detect(self, GST_VIDEO_FRAME_PLANE_DATA(frame, 0), NULL, size);
}

static void gst_color_detect_finalize(GObject *object) {
  GstColorDetect *self = GST_COLOR_DETECT(object);
  g_free(self->current_color);
  g_mutex_clear(&self->lock);
  G_OBJECT_CLASS(gst_color_detect_parent_class)->finalize(object);
}

static void gst_color_detect_class_init(GstColorDetectClass *klass) {
  GObjectClass *gobject = G_OBJECT_CLASS(klass);
  GstElementClass *element = GST_ELEMENT_CLASS(klass);
  GstBaseTransformClass *trans = GST_BASE_TRANSFORM_CLASS(klass);
  GstVideoFilterClass *vfilter = GST_VIDEO_FILTER_CLASS(klass);
  gobject->set_property = gst_color_detect_set_property;
  gobject->get_property = gst_color_detect_get_property;
  gobject->finalize = gst_color_detect_finalize;
  const GParamFlags f = (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS | GST_PARAM_MUTABLE_PLAYING);
  g_object_class_install_property(gobject, PROP_QUALITY,
      g_param_spec_uint("quality", "Quality of an output colors", "A step in pixels to improve performance", 0, 10, 10, f));
  g_object_class_install_property(gobject, PROP_MAX_COLORS,
      g_param_spec_uint("max-colors", "Number of colors in the output palette", "Actual colors count can be lower depending on the image", 2, 255, 2, f));
  gst_element_class_set_static_metadata(element, "Dominant color detection", "Filter/Video", "Detects the dominant color of a video",
                                        "Philippe Normand <philn@igalia.com>");
  gst_element_class_add_static_pad_template(element, &sink_template);
  gst_element_class_add_static_pad_template(element, &src_template);
  trans->start = gst_color_detect_start;
  trans->stop = gst_color_detect_stop;
  trans->transform_ip = gst_color_detect_transform_ip; /* GstVideoFilter's transform_ip is reached by chaining up */
  trans->passthrough_on_same_caps = TRUE;    /* imp.rs:249 */
  trans->transform_ip_on_passthrough = TRUE; /* imp.rs:250 */
  vfilter->set_info = gst_color_detect_set_info;
  vfilter->transform_frame_ip = gst_color_detect_transform_frame_ip; /* only the ip slot == BaseTransformMode::AlwaysInPlace */
  GST_DEBUG_CATEGORY_INIT(gst_color_detect_debug, "colordetect", 0, "Dominant color detection");
}

static void gst_color_detect_init(GstColorDetect *self) {
  g_mutex_init(&self->lock);
  self->quality = 10;   /* DEFAULT_QUALITY (imp.rs:19) */
  self->max_colors = 2; /* DEFAULT_MAX_COLORS (imp.rs:20) */
}

gboolean gst_color_detect_register(GstPlugin *plugin) {
  return gst_element_register(plugin, "colordetect", GST_RANK_NONE, GST_TYPE_COLOR_DETECT); /* colordetect/mod.rs */
}
