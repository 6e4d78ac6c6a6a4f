// group.hip — frames of MANY streams in few launches: the dispatcher behind mi355_group_*.
//
// GstBaseTransform hands every element ONE buffer per call (video/hsv/src/hsvfilter/imp.rs:323-376,
// video/colorlut/src/colorlut/imp.rs:203-223), so N streams through `hsvfilter ! colorlut` are 2 N launches per frame period,
// each with its own ramp and tail (a one-frame hsvfilter launch: 16.5 us against 10.7 us for an eighth of an eight-frame
// launch; 32 streams: 34 k frames/s against 45 k batched, profiles/r03_launch_size.txt). A group collects what the streams
// submit - {stream's context, frame in, frame out, geometry, hsv settings of that frame} - and issues it as multi-frame
// launches: the frames of up to `max_batch` streams that agree in geometry, format, settings and LUT go to ONE hsvfilter launch
// and ONE colorlut launch (blockIdx -> frame -> base pointer from the kernel arguments; hsv_kernels.hip, colorlut_kernels.hip).
//   * submit never blocks and never launches on its own unless max_batch frames are pending;
//   * mi355_group_wait(ticket) flushes what is pending if that ticket has not been launched yet, then waits for its batch -
//     an element that works one frame deep (submit frame n, wait for frame n-1: gst/gstcolorlut.c) therefore fills batches
//     with the frames the other streams submitted in between, and a lone stream degenerates to today's two launches;
//   * order: batches run in submission order on the group's own HIP stream and hold at most one frame per stream, so frames of
//     one stream run in order; a frame starts after the work its context's stream held at submit time (an event, only if the
//     stream held any); what the context's stream does NEXT is ordered after a frame by mi355_group_order_after (one stream
//     wait, asked for by who needs it: a download) or by the host wait - not by default: eight barrier packets behind every
//     batch cost more than the batching saves (32 streams: 31 k frames/s with them, see DESIGN);
//   * results are the two element launches', bit for bit (same arithmetic, same table);
//   * frames the batched kernels do not take (padded rows, 3-byte formats, no table) run through their context's own path,
//     in order.
// Seven more queues live beside the filter batches, each with its own HIP stream(s), pending list, rendezvous and stats, and none
// touching another. They are SET QUEUES: one protocol written once - SetQueue<Kind>: submit's tail, flush in sets of up to 32 of
// one class in submission order, each set dealt out to the kind's lanes, the lingering wait, collect-once results per lane,
// retire, stats, destroy - with seven kinds:
//   * CmpKind, videocompare pairs (submit_compare). The one kind with classes (algorithm, geometry, format, Dssim form) and lanes:
//     a set's pairs, sorted by reference frame, go out as contiguous shares on up to 16 streams.
//   * CdKind, colordetect frames (submit_colordetect).
//   * YdKind, decoder tensors (submit_yolodec): tensors of independent yolov8tensordec2 / yoloxtensordec instances - own shape,
//     layout, settings - as at most three launches over job tables and one download, yolodec.hip. The raw head maps of independent
//     yoloxinference instances (submit_yolox_head) are members of the SAME queue: a YdTensor of the kind MI355_YOLO_X_HEAD with
//     the submit's copy of its levels; they cost a set one upload of their level tables and two launches more, yolox_head.hip.
//     RGB frames for a shared, finalized yoloxinference net (submit_yolox_infer) are members of the same queue too: a YdTensor of
//     the kind MI355_YOLO_X_INFER. A set converts all of them in one launch and runs ONE forward per class (net, H, W) in an
//     activation lane of the queue's own (yolox_net.hip: YxLanes); from the score launch on they are heads.
//   * HnKind, hand tensors (submit_handdec_palm / _landmarks): tensors of independent handdetectiontensordec /
//     handlandmarktensordec instances - own shape and settings - as at most two launches over job tables, no upload and one
//     download, handdec.hip.
//   * HdKind and HfKind, hsvdetector and hsvfilter frames (submit_hsvdetect, submit_hsvfilter): frames of independent instances -
//     own size, strides, formats, settings - as at most two launches over a job table, hsv_kernels.hip. Both are FrameKind<traits>:
//     written on the device, nothing to bring back. hsvfilter works IN PLACE and is the one kind whose members must not share
//     bytes within a launch: its submit entry launches what is pending in front of a frame that overlaps a pending one, and the
//     sets of the queue's one stream run in order.
//   * ClKind, colorlut frames (submit_colorlut): a third FrameKind, source to destination - own size, strides, format and the LUT
//     of the member's context - as at most two launches over a job table, colorlut_group.hip. Its submit entry launches what is
//     pending in front of a frame that writes what a pending one reads or writes, or reads what a pending one writes.
// A further kind is a struct beside these - payload, result, kSetMax, its names, ensure, plan (PayloadPlan, if the launch reads
// the payloads as they are), the size of its pinned block (if any), launch, result, failed, destroy; OneLane, or its own same_class
// / split / lanes - or, for frames written on the device, the traits of a FrameKind. It is a SetQueue<Kind> member of mi355_group
// and a line in for_each_queue_but_compare, which is how flush, wait_all, destroy and the foreign-ticket refusal reach it; its entry points
// check their own arguments and take their rendezvous, stats and (status-only) wait bodies from queue_set_rendezvous, queue_stats
// and queue_wait_status. Nothing of the protocol is written again. The filter batches alone are their own code: one frame per
// stream and batch, the non-batchable path and order_after are not this protocol.
// The group has ONE mutex, ticket sequence, event free list and last_error (GroupCore); every queue uses those. Tickets are one
// sequence; a wait entry refuses a ticket of another queue.
// No persistent kernel: nothing here can hang the GPU waiting for the host, a launch is a launch.
#include "internal.hpp"

#include <chrono>
#include <condition_variable>
#include <algorithm>
#include <cstring>
#include <deque>
#include <mutex>
#include <unordered_map>
#include <vector>

using namespace mi355;

namespace {

struct Desc {
  mi355_ctx *ctx;
  uint8_t *src, *dst;
  int width, height, stride, format;
  mi355_hsv_settings hs;
  const uint32_t *table;  // the context's memoised colorlut table (nullptr: not batchable)
  // ... and a reference to it, held until the frame's batch has retired: the context may move on to other settings (or another
  // LUT) before this frame has been launched or has finished, and a table somebody else still refers to is never rebuilt in place
  // (colorlut_kernels.hip: shared_table_acquire takes that branch only for use_count() == 1) nor freed
  std::shared_ptr<void> table_ref;
  bool batchable;
  bool fused;             // one launch through the composed hsv+lut table, source left untouched (mi355_group_submit_fused)
  uint64_t ticket;
  hipEvent_t ready;       // recorded on ctx->stream at submit
};

struct Batch {
  uint64_t seq;                   // launch order on the group's stream: batch n is done => every batch before it is
  std::vector<uint64_t> tickets;  // the frames it carries (not a contiguous range: an incompatible frame waits for the next batch)
  hipEvent_t done;
  int waiters;  // threads inside hipEventSynchronize(done) right now: the event is not recycled under them
  std::shared_ptr<void> table_ref;  // the table its launches read (see Desc)
};

// ---- what every queue of a group shares: ONE lock, ticket sequence, event free list and last_error
struct GroupCore {
  int device = 0;
  std::mutex mu;
  std::vector<hipEvent_t> events;  // free list
  uint64_t next_ticket = 1;
  std::string last_error;
};

hipEvent_t take_event(GroupCore *g) {
  if (!g->events.empty()) { hipEvent_t e = g->events.back(); g->events.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return e;
}

int fail(GroupCore *g, int status, const std::string &msg) {
  g->last_error = msg;
  return status;
}

// What is submitted starts after what ctx's stream holds now (an upload, a filter, the table build): *ready is recorded there. A
// stream that holds nothing - the common case for a stream that only ever submits here - needs no event (*ready = nullptr): every
// cross-stream wait is a barrier packet the command processor resolves in microseconds, eight of them in front of a 90 us launch
// are a bubble. g->mu held.
int record_ready(GroupCore *g, mi355_ctx *ctx, hipEvent_t *ready) {
  *ready = nullptr;
  if (hipStreamQuery(ctx->stream) == hipSuccess) return MI355_OK;
  (void)hipGetLastError();
  hipEvent_t e = take_event(g);
  if (!e || hipEventRecord(e, ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    if (e) g->events.push_back(e);
    return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
  }
  *ready = e;
  return MI355_OK;
}

// The host wait for the batch / set `seq` of `sets`. The lock is NOT held while waiting: other streams' threads keep submitting,
// and `waiters` keeps the event from being recycled under the waiter. `lk` owns g->mu on entry and on return.
enum class Waited { kNothing /* no such set: retired already */, kDone, kFailed };
template <class S>
Waited wait_seq_unlocking(std::deque<S> &sets, uint64_t seq, std::unique_lock<std::mutex> &lk) {
  S *mine = nullptr;
  for (S &s : sets)
    if (s.seq == seq) { mine = &s; break; }
  if (!mine) return Waited::kNothing;
  const hipEvent_t ev = mine->done;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (S &s : sets)
    if (s.seq == seq) { s.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return Waited::kFailed; }
  return Waited::kDone;
}

// ------------------------------------------------------------------ the set queue (SetQueue<Kind>) and its seven kinds
// A kind is what differs between the queues: what is submitted (Payload), what a wait takes (Result), what a launch reads (Plan),
// what a set in flight owns (SetData: its pinned `block` and what `result` needs besides), how a set is launched and read back, how
// large its block has to be, the resources of first use - and which pending items may share a launch set (same_class) and how
// what was taken is dealt out to the kind's streams (split: parts, each with a lane). The protocol is below.

template <class Payload>
struct QItem {
  Payload p;
  uint64_t ticket;
  hipEvent_t ready;  // recorded on the submitting context's stream (nullptr: the stream held nothing, or nothing will be read)
};

// items [begin, end) of what a flush took, as one launch on the stream of `lane`
struct Part { int lane; size_t begin, end; };

// A pinned result block, and a kind's free list of them. Sets' results may differ in size by orders of magnitude (the decoder's:
// min(max_dets, N) records per tensor), so blocks are sized: `take` hands out a free one that is large enough, else a new one -
// and a free one that is too small makes room, or the pool would keep every size it saw. Where every request has one size (the
// other kinds) that is pop-or-allocate: a launch set allocates only when more sets are in flight than ever before.
struct PinnedBlock { void *h = nullptr; size_t bytes = 0; };
struct BlockPool {
  std::vector<PinnedBlock> free;
  static bool alloc(size_t bytes, PinnedBlock *b) {
    const size_t want = (bytes + 4095) / 4096 * 4096;
    if (hipHostMalloc(&b->h, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *b = PinnedBlock{}; return false; }
    b->bytes = want;
    return true;
  }
  bool take(size_t bytes, PinnedBlock *b) {
    for (size_t i = 0; i < free.size(); i++)
      if (free[i].bytes >= bytes) {
        *b = free[i];
        free.erase(free.begin() + (std::ptrdiff_t)i);
        return true;
      }
    if (!free.empty()) {
      (void)hipHostFree(free.back().h);
      free.pop_back();
    }
    return alloc(bytes, b);
  }
  void give(PinnedBlock *b) {
    if (b->h) free.push_back(*b);
    *b = PinnedBlock{};
  }
  // the blocks of first use: the sets a stream of submits has in flight before anybody collects
  bool prefill(size_t n, size_t bytes) {
    while (free.size() < n) {
      PinnedBlock b;
      if (!alloc(bytes, &b)) return false;
      free.push_back(b);
    }
    return true;
  }
  void destroy() {
    for (PinnedBlock &b : free) (void)hipHostFree(b.h);
    free.clear();
  }
};

// What the kinds with ONE stream share: everything pending is one class, and what a flush took is one part on lane 0.
template <class Payload>
struct OneLane {
  static constexpr int kLanesMax = 1;
  hipStream_t stream = nullptr;
  int lanes() const { return 1; }
  hipStream_t lane_stream(int) const { return stream; }
  static bool same_class(const Payload &, const Payload &) { return true; }
  int split(std::vector<QItem<Payload>> &all, Part *parts) const {
    parts[0] = Part{0, 0, all.size()};
    return 1;
  }
};

int queue_stream(GroupCore *g, hipStream_t *stream, const char *name) {
  if (*stream) return MI355_OK;
  if (hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    *stream = nullptr;
    return fail(g, MI355_ERR_HIP, std::string("group: no stream for the ") + name + " queue");
  }
  return MI355_OK;
}

int device_cus(int device) {
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) (void)hipGetLastError();
  return n_cu > 0 ? n_cu : 256;
}

// What the kinds whose launch reads the payloads as they were submitted share (CdKind, FrameKind): the plan is a copy of them.
template <class Payload, int N>
struct PayloadPlan : OneLane<Payload> {
  struct Plan { Payload frames[N]; };
  int plan(const QItem<Payload> *take, size_t n, Plan *p, std::string *) const {
    for (size_t i = 0; i < n; i++) p->frames[i] = take[i].p;
    return MI355_OK;
  }
};

// ---- colordetect across independent element instances (mi355_group_submit_colordetect): one flat device plane per submit; its
// palette comes back through the set's pinned block. Consecutive sets on the queue's stream share the device scratch.
struct CdOut { int status, n_colors; uint8_t rgb[255 * 3]; };
constexpr int kCdBlocksAtFirstUse = 4;  // pinned result blocks = launch sets in flight before one more has to be allocated
struct CdKind : PayloadPlan<CdFrame, kCdSetMax> {
  using Payload = CdFrame;
  using Result = CdOut;
  struct SetData { PinnedBlock block; };  // the set's results (colordetect_set_result) until it is collected
  static constexpr int kSetMax = kCdSetMax;
  static constexpr const char *kName = "colordetect", *kItem = "colordetect frame", *kWaitEntry = "mi355_group_wait_colordetect";
  CdSetScratch *scratch = nullptr;
  int n_cu = 256;
  BlockPool blocks;  // all of colordetect_set_block_bytes()

  bool set_up() const { return scratch != nullptr; }
  // stream, device scratch and the first pinned blocks: at the first submit, never inside a launch set
  int ensure(GroupCore *g) {
    if (scratch) return MI355_OK;
    n_cu = device_cus(g->device);
    if (int rc = queue_stream(g, &stream, kName)) return rc;
    if (!blocks.prefill(kCdBlocksAtFirstUse, colordetect_set_block_bytes())) return fail(g, MI355_ERR_OUT_OF_MEMORY, "group: no pinned result blocks for the colordetect queue");
    int st = MI355_OK;
    std::string err;
    scratch = colordetect_set_scratch_new(stream, &st, &err);
    return scratch ? MI355_OK : fail(g, st, "group: " + err);
  }
  size_t block_bytes(const Plan &) const { return colordetect_set_block_bytes(); }
  int launch(int, const Plan &p, size_t n, SetData *d, int *launches, std::string *err) {
    return colordetect_launch_set(scratch, stream, n_cu, p.frames, (int)n, d->block.h, launches, err);
  }
  void launched(const GroupCore *, const Plan &, size_t) const {}
  void result(const SetData &d, size_t i, CdOut *o) const {
    o->status = MI355_OK;
    colordetect_set_result(d.block.h, (int)i, o->rgb, &o->n_colors);
  }
  static void failed(const CdFrame &, int rc, CdOut *o) { o->status = rc; o->n_colors = 0; }
  static int status(const CdOut &o) { return o.status; }
  void destroy() {
    colordetect_set_scratch_free(scratch);
    (void)hipStreamDestroy(stream);
    blocks.destroy();
  }
};

// ---- frames written on the device, across independent element instances: one device frame per submit, and nothing comes back but
// the launch's status - a set owns NO pinned block and the queue no scratch. Three kinds, each a few lines of traits (the frame, its
// names, its launch-set function in hsv_kernels.hip and the bytes a frame's launch writes):
//   HdKind  hsvdetector (mi355_group_submit_hsvdetect): source to destination.
//   HfKind  hsvfilter (mi355_group_submit_hsvfilter): IN PLACE, so the frames of a set must not overlap, which the submit entry sees
//           to (it launches what is pending in front of a frame that overlaps a pending one).
struct HdTraits {
  using Frame = HdFrame;
  static constexpr int kSetMax = kHdSetMax;
  static constexpr const char *kName = "hsvdetector", *kItem = "hsvdetector frame", *kWaitEntry = "mi355_group_wait_hsvdetect";
  static constexpr auto kLaunchSet = hsvdetect_launch_set;
  static const void *written(const HdFrame &f, size_t *bytes) { *bytes = (size_t)f.dst_stride * (size_t)f.height; return f.dst; }
};
struct HfTraits {
  using Frame = HfFrame;
  static constexpr int kSetMax = kHfSetMax;
  static constexpr const char *kName = "hsvfilter", *kItem = "hsvfilter frame", *kWaitEntry = "mi355_group_wait_hsvfilter";
  static constexpr auto kLaunchSet = hsvfilter_launch_set;
  static const void *written(const HfFrame &f, size_t *bytes) { *bytes = (size_t)f.stride * (size_t)f.height; return f.data; }
};
// ClKind  colorlut (mi355_group_submit_colorlut): source to destination through the LUT the member's context held at submit
//         (borrowed until the wait returns); a frame that meets a pending one launches what is pending first, as hsvfilter's does.
struct ClTraits {
  using Frame = ClFrame;
  static constexpr int kSetMax = kClSetMax;
  static constexpr const char *kName = "colorlut", *kItem = "colorlut frame", *kWaitEntry = "mi355_group_wait_colorlut";
  static constexpr auto kLaunchSet = colorlut_launch_set;
  static const void *written(const ClFrame &f, size_t *bytes) { *bytes = (size_t)f.dst_stride * (size_t)f.height; return f.dst; }
};
template <class T>
struct FrameKind : PayloadPlan<typename T::Frame, T::kSetMax> {
  using Payload = typename T::Frame;
  using Result = int;  // the status
  using Plan = typename PayloadPlan<Payload, T::kSetMax>::Plan;
  struct SetData { PinnedBlock block; };  // (never taken: block_bytes is 0)
  static constexpr int kSetMax = T::kSetMax;
  static constexpr const char *kName = T::kName, *kItem = T::kItem, *kWaitEntry = T::kWaitEntry;
  int n_cu = 256;
  BlockPool blocks;  // (stays empty)

  bool set_up() const { return this->stream != nullptr; }
  // the queue's stream is all it has, so first use is keyed on it: at the first submit, never inside a launch set
  int ensure(GroupCore *g) {
    if (this->stream) return MI355_OK;
    n_cu = device_cus(g->device);
    return queue_stream(g, &this->stream, kName);
  }
  size_t block_bytes(const Plan &) const { return 0; }
  int launch(int, const Plan &p, size_t n, SetData *, int *launches, std::string *err) { return T::kLaunchSet(this->stream, n_cu, p.frames, (int)n, launches, err); }
  // what the element behind finds on-die, as the lone entry records it: what every frame with a pixel writes, once the set has gone out
  void launched(const GroupCore *g, const Plan &p, size_t n) const {
    for (size_t i = 0; i < n; i++) {
      size_t bytes = 0;
      const void *at = T::written(p.frames[i], &bytes);
      if (p.frames[i].width > 0 && p.frames[i].height > 0) note_written(g->device, at, bytes);
    }
  }
  void result(const SetData &, size_t, int *o) const { *o = MI355_OK; }
  static void failed(const Payload &, int rc, int *o) { *o = rc; }
  static int status(int o) { return o; }
  void destroy() { (void)hipStreamDestroy(this->stream); }
};
using HdKind = FrameKind<HdTraits>;
using HfKind = FrameKind<HfTraits>;
using ClKind = FrameKind<ClTraits>;

// ---- yolov8tensordec2 / yoloxtensordec across independent element instances (mi355_group_submit_yolodec): one device tensor per
// submit; its kept count and records come back through the set's pinned block. Consecutive sets share the device scratch.
struct YdOut { int status; uint32_t n_dets, max_dets; std::vector<mi355_yolo_det> dets; };   // dets: the first min(n_dets, max_dets)
struct YdSlot { uint32_t num_candidates, max_dets; uint64_t det_offset; };
struct YdKind : OneLane<YdTensor> {
  using Payload = YdTensor;
  using Result = YdOut;
  struct Plan { YdTensor tensors[kYdSetMax]; YdSetPlan set; };
  struct SetData {
    // the set's own results until it is collected, and behind them the tables of its heads (h == nullptr: no member had a candidate)
    PinnedBlock block;
    std::vector<YdSlot> slots;   // its tensors, by job (as the set's tickets are)
  };
  static constexpr int kSetMax = kYdSetMax;
  static constexpr const char *kName = "decoder", *kItem = "decoder tensor", *kWaitEntry = "mi355_group_wait_yolodec";
  YdSetScratch *scratch = nullptr;
  BlockPool blocks;  // sized by the sets' results
  // the heads among the members (mi355_group_yolox_head_stats): heads launched, sets that held one, table uploads, head kernel launches
  uint64_t n_heads = 0, n_head_sets = 0, n_head_uploads = 0, n_head_launches = 0;
  int last_head_counts[3] = {0, 0, 0};   // of the set `launch` has just sent out; counted by `launched`, i.e. once the set stands
  // the infer members (mi355_group_yolox_infer_stats): frames, forwards (classes), frames of the largest forward, kernel launches of
  // conversions and forwards; their lanes, made with the scratch and freed by destroy; the net (by serial) of every infer ticket
  // that its wait has not taken yet (release_yolox_net refuses a net that one of them names)
  uint64_t n_infer = 0, n_forwards = 0, n_largest_forward = 0, n_infer_launches = 0;
  int last_infer_counts[4] = {0, 0, 0, 0};
  YxLanes *net_lanes = nullptr;
  int n_cu = 256;
  std::unordered_map<uint64_t, uint64_t> infer_tickets;

  // flush, wait_all and destroy launch for this queue only once the scratch exists: a stream alone (the scratch could not be made)
  // has accepted nothing
  bool set_up() const { return scratch != nullptr; }
  // the queue's stream and scratch: at the first submit, never inside a launch set
  int ensure(GroupCore *g) {
    if (scratch) return MI355_OK;
    if (int rc = queue_stream(g, &stream, kName)) return rc;
    int st = MI355_OK;
    std::string err;
    if (!net_lanes) net_lanes = yolox_lanes_new();
    n_cu = device_cus(g->device);
    scratch = yolodec_set_scratch_new(&st, &err);
    return scratch ? MI355_OK : fail(g, st, "group: " + err);
  }
  // the set's layout, before anything is taken for it: the plan the launch itself uses says how large the set's block has to be
  int plan(const QItem<YdTensor> *take, size_t n, Plan *p, std::string *err) const {
    for (size_t i = 0; i < n; i++) p->tensors[i] = take[i].p;
    const int rc = yolodec_plan_set(p->tensors, (int)n, &p->set);
    if (rc) *err = "group: bad decoder set";
    return rc;
  }
  // a set without a candidate has nothing to copy: it takes no block (and still gets its event and its set)
  size_t block_bytes(const Plan &p) const { return p.set.totals[2] ? yolodec_set_block_bytes(p.set.totals[5], p.set.totals[7], p.set.infer_totals[1]) : 0; }
  int launch(int, const Plan &p, size_t n, SetData *d, int *launches, std::string *err) {
    for (size_t i = 0; i < n; i++) d->slots.push_back(YdSlot{p.tensors[i].num_candidates, p.tensors[i].max_dets, p.set.det_off[i]});
    return yolodec_launch_set(scratch, stream, p.tensors, (int)n, p.set, d->block.h, d->block.bytes, launches, last_head_counts, err, net_lanes, n_cu, last_infer_counts);
  }
  void launched(const GroupCore *, const Plan &, size_t) {
    n_heads += (uint64_t)last_head_counts[0];
    n_head_sets += last_head_counts[0] ? 1 : 0;
    n_head_uploads += (uint64_t)last_head_counts[1];
    n_head_launches += (uint64_t)last_head_counts[2];
    n_infer += (uint64_t)last_infer_counts[0];
    n_forwards += (uint64_t)last_infer_counts[1];
    n_largest_forward = std::max(n_largest_forward, (uint64_t)last_infer_counts[2]);
    n_infer_launches += (uint64_t)last_infer_counts[3];
  }
  // counts and records MOVE out of the pinned block: a later, larger set cannot overwrite what an earlier ticket has not collected
  void result(const SetData &d, size_t i, YdOut *o) const {
    const uint32_t *h_n = static_cast<const uint32_t *>(d.block.h);
    const mi355_yolo_det *h_dets = d.block.h ? reinterpret_cast<const mi355_yolo_det *>(static_cast<const uint8_t *>(d.block.h) + kYdCountsBytes) : nullptr;
    const YdSlot &sl = d.slots[i];
    o->status = MI355_OK;
    o->max_dets = sl.max_dets;
    o->n_dets = sl.num_candidates && h_n ? h_n[i] : 0;   // a tensor without candidates had no job
    const uint32_t cap = sl.max_dets < sl.num_candidates ? sl.max_dets : sl.num_candidates;
    const uint32_t w = o->n_dets < cap ? o->n_dets : cap;
    if (w) o->dets.assign(h_dets + sl.det_offset, h_dets + sl.det_offset + w);
  }
  static void failed(const YdTensor &t, int rc, YdOut *o) { o->status = rc; o->n_dets = 0; o->max_dets = t.max_dets; }
  static int status(const YdOut &o) { return o.status; }
  void destroy() {
    yolodec_set_scratch_free(scratch);
    yolox_lanes_free(net_lanes);   // (the queue's stream has been waited for)
    (void)hipStreamDestroy(stream);
    blocks.destroy();
  }
};

// ---- handdetectiontensordec / handlandmarktensordec across independent element instances (mi355_group_submit_handdec_palm /
// _landmarks): one device tensor per submit; its count and records come back through the set's pinned block. Consecutive sets share
// the device slab, which holds one set's results at their maximum - so the pinned blocks have ONE size, as colordetect's have.
struct HnOut { int status, decoder; uint32_t n_hands; std::vector<mi355_hand_det> dets; std::vector<mi355_hand_keypoints> kps; };   // the first n_hands
struct HnSlot { int decoder; uint32_t rows, kp_slot; };
constexpr int kHnBlocksAtFirstUse = 4;  // pinned result blocks = launch sets in flight before one more has to be allocated
struct HnKind : OneLane<HnTensor> {
  using Payload = HnTensor;
  using Result = HnOut;
  struct Plan { HnTensor tensors[kHnSetMax]; HnSetPlan set; };
  struct SetData {
    PinnedBlock block;           // the set's own results until it is collected (h == nullptr: no tensor had rows)
    std::vector<HnSlot> slots;   // its tensors, by job (as the set's tickets are)
  };
  static constexpr int kSetMax = kHnSetMax;
  static constexpr const char *kName = "hand decoder", *kItem = "hand tensor", *kWaitEntry = "mi355_group_wait_handdec";
  HnSetScratch *scratch = nullptr;
  BlockPool blocks;  // all of handdec_set_block_bytes()

  bool set_up() const { return scratch != nullptr; }
  // stream, device slab and the first pinned blocks: at the first submit, never inside a launch set
  int ensure(GroupCore *g) {
    if (scratch) return MI355_OK;
    if (int rc = queue_stream(g, &stream, kName)) return rc;
    if (!blocks.prefill(kHnBlocksAtFirstUse, handdec_set_block_bytes())) return fail(g, MI355_ERR_OUT_OF_MEMORY, "group: no pinned result blocks for the hand decoder queue");
    int st = MI355_OK;
    std::string err;
    scratch = handdec_set_scratch_new(&st, &err);
    return scratch ? MI355_OK : fail(g, st, "group: " + err);
  }
  // the set's layout, by the plan the launch itself uses: which tensors have a block, the landmark tensors' keypoint slots
  int plan(const QItem<HnTensor> *take, size_t n, Plan *p, std::string *err) const {
    for (size_t i = 0; i < n; i++) p->tensors[i] = take[i].p;
    const int rc = handdec_plan_set(p->tensors, (int)n, &p->set);
    if (rc) *err = "group: bad hand decoder set";
    return rc;
  }
  // a set without a row has nothing to copy: it takes no block (and still gets its event and its set)
  size_t block_bytes(const Plan &p) const { return p.set.totals[3] ? handdec_set_block_bytes() : 0; }
  int launch(int, const Plan &p, size_t n, SetData *d, int *launches, std::string *err) {
    for (size_t i = 0; i < n; i++) d->slots.push_back(HnSlot{p.tensors[i].decoder, p.tensors[i].rows, p.set.kp_slot[i]});
    return handdec_launch_set(scratch, stream, p.tensors, (int)n, p.set, d->block.h, d->block.h ? handdec_set_block_bytes() : 0, launches, err);
  }
  void launched(const GroupCore *, const Plan &, size_t) const {}
  // count and records MOVE out of the pinned block: the block is free for a later set once this one is collected
  void result(const SetData &d, size_t i, HnOut *o) const {
    const HnSlot &sl = d.slots[i];
    mi355_hand_det dets[MI355_HAND_MAX];
    mi355_hand_keypoints kps[MI355_HAND_MAX];
    o->status = MI355_OK;
    o->decoder = sl.decoder;
    handdec_set_result(d.block.h, (int)d.slots.size(), (int)i, sl.decoder, sl.rows, sl.kp_slot, dets, kps, &o->n_hands);
    o->dets.assign(dets, dets + o->n_hands);
    if (sl.decoder == 1) o->kps.assign(kps, kps + o->n_hands);
  }
  static void failed(const HnTensor &t, int rc, HnOut *o) { o->status = rc; o->decoder = t.decoder; o->n_hands = 0; }
  static int status(const HnOut &o) { return o.status; }
  void destroy() {
    handdec_set_scratch_free(scratch);
    (void)hipStreamDestroy(stream);
    blocks.destroy();
  }
};

// ---- videocompare across independent element instances (mi355_group_submit_compare): one (reference frame, frame) pair per
// submit; its distance (and Blockhash's two hashes) come back through the part's pinned block. The one kind with classes and lanes:
// a launch set holds pairs of one class, and its pairs are dealt out to `n_lanes` contexts (streams) - the Dssim kernels are
// VALU-bound at ~80 % busy when one runs alone, and a second stream's launches fill its tails and launch boundaries (32 4K pairs:
// 1.48 k comparisons/s on one stream, 1.84 k over eight); what the dispatcher removes is the per-comparison host round trip, not
// the overlap.
struct CmpPair {
  const uint8_t *ref, *frame;
  int width, height, stride, format, algo, translucent, fast;   // translucent, fast: the submitting context's Dssim settings
};
struct CmpResult { int status; double distance; uint64_t hashes[2]; };
constexpr int kCmpMaxBatch = 32;                      // pairs per launch set (a Dssim pair keeps 44 MB of maps until its batch is reduced)
constexpr int kCmpMaxLanes = 16;                      // HIP streams the pairs of one launch set are dealt out to
constexpr size_t kCmpBlockBytes = 64 * 15 * 8 + 1024; // one pinned result block
struct CmpKind {
  using Payload = CmpPair;
  using Result = CmpResult;
  struct Plan { CmpPair first; const uint8_t *refs[kCmpMaxBatch], *frames[kCmpMaxBatch]; };
  struct SetData {
    PinnedBlock block;           // Dssim [n][15] doubles / Blockhash [2 n] u64 (reference hashes, then frame hashes)
    int algo = 0, width = 0, height = 0, n = 0;
    std::vector<double> scores;  // Dssim: the part's n distances, reduced from the block when its first result is taken
  };
  static constexpr int kSetMax = kCmpMaxBatch, kLanesMax = kCmpMaxLanes;
  static constexpr const char *kName = "compare", *kItem = "pair";   // (no kWaitEntry: no other entry refuses a pair's ticket by name)
  mi355_ctx *alane[kCmpMaxLanes] = {nullptr};        // a context (stream, Dssim scratch) per lane
  int n_lanes = 8;
  uint32_t *d_hash_sums[kCmpMaxLanes] = {nullptr};   // Blockhash scratch per lane: [2 kCmpMaxBatch][64] u32 + [2 kCmpMaxBatch] u64
  BlockPool blocks;  // all of kCmpBlockBytes

  bool set_up() const { return alane[0] != nullptr; }
  int lanes() const { return n_lanes; }
  hipStream_t lane_stream(int lane) const { return alane[lane] ? alane[lane]->stream : nullptr; }
  // the lane contexts and their Blockhash scratch: at the first submit, all of them or none
  int ensure(GroupCore *g) {
    if (set_up()) return MI355_OK;
    int st = MI355_OK;
    for (int l = 0; l < n_lanes && !st; l++) {
      alane[l] = mi355_ctx_create(g->device, &st);
      if (!alane[l] && !st) st = MI355_ERR_HIP;
      if (!st && hipMalloc((void **)&d_hash_sums[l], (size_t)2 * kCmpMaxBatch * (64 * 4 + 8)) != hipSuccess) { (void)hipGetLastError(); st = MI355_ERR_OUT_OF_MEMORY; }
    }
    if (!st) return MI355_OK;
    free_lanes();
    return fail(g, st, "group: no contexts for the compare queue");
  }
  void free_lanes() {
    for (int l = 0; l < kCmpMaxLanes; l++) {
      if (d_hash_sums[l]) (void)hipFree(d_hash_sums[l]);
      if (alane[l]) mi355_ctx_destroy(alane[l]);
      d_hash_sums[l] = nullptr; alane[l] = nullptr;
    }
  }
  static bool same_class(const CmpPair &a, const CmpPair &b) {
    return a.algo == b.algo && a.width == b.width && a.height == b.height && a.stride == b.stride && a.format == b.format && a.translucent == b.translucent && a.fast == b.fast;
  }
  // pairs that share a reference frame next to each other (videocompare with several pads: the reference is hashed once), then
  // contiguous shares for the lanes
  int split(std::vector<QItem<CmpPair>> &all, Part *parts) const {
    std::stable_sort(all.begin(), all.end(), [](const QItem<CmpPair> &a, const QItem<CmpPair> &b) { return (uintptr_t)a.p.ref < (uintptr_t)b.p.ref; });
    const int total = (int)all.size();
    const int shares = total < n_lanes ? total : n_lanes;
    int n_parts = 0, begin = 0;
    for (int lane = 0; lane < shares; lane++) {
      int end = (int)((long long)total * (lane + 1) / shares);
      // a reference frame is not split over two lanes
      while (end < total && end > begin && all[end].p.ref == all[end - 1].p.ref) end++;
      if (end <= begin) continue;
      parts[n_parts++] = Part{lane, (size_t)begin, (size_t)end};
      begin = end;
    }
    return n_parts;
  }
  int plan(const QItem<CmpPair> *take, size_t n, Plan *p, std::string *) const {
    p->first = take[0].p;   // a part holds pairs of one class only (same_class)
    for (size_t i = 0; i < n; i++) { p->refs[i] = take[i].p.ref; p->frames[i] = take[i].p.frame; }
    return MI355_OK;
  }
  size_t block_bytes(const Plan &) const { return kCmpBlockBytes; }
  int launch(int lane, const Plan &p, size_t n, SetData *d, int *, std::string *err) {
    const CmpPair &c = p.first;
    mi355_ctx *a = alane[lane];
    PixFmt fmt;
    (void)pixfmt_of(c.format, &fmt);
    d->algo = c.algo; d->width = c.width; d->height = c.height; d->n = (int)n;
    int rc = MI355_OK;
    if (c.algo == MI355_HASH_DSSIM) {
      a->dssim_translucent = c.translucent;
      a->dssim_fast = c.fast;
      rc = dssim_compare_pairs_enqueue(a, p.refs, p.frames, (int)n, c.stride, c.width, c.height, fmt.pixel_stride, (double *)d->block.h);
    } else {
      const uint8_t *both[2 * kCmpMaxBatch];
      std::copy(p.refs, p.refs + n, both);
      std::copy(p.frames, p.frames + n, both + n);
      unsigned long long *d_hashes = (unsigned long long *)(d_hash_sums[lane] + (size_t)2 * kCmpMaxBatch * 64);
      rc = blockhash_enqueue(a, both, 2 * (int)n, c.stride, c.width, c.height, fmt.pixel_stride, d_hash_sums[lane], d_hashes);
      if (!rc && hipMemcpyAsync(d->block.h, d_hashes, (size_t)2 * n * 8, hipMemcpyDeviceToHost, a->stream) != hipSuccess) rc = MI355_ERR_HIP;
    }
    if (rc) *err = a->last_error;
    return rc;
  }
  void launched(const GroupCore *, const Plan &, size_t) const {}
  void result(SetData &d, size_t i, CmpResult *o) const {
    if (d.algo == MI355_HASH_DSSIM) {
      if (d.scores.empty()) {
        d.scores.resize((size_t)d.n);
        dssim_scores_from_slots(d.width, d.height, (const double *)d.block.h, d.n, d.scores.data());
      }
      *o = CmpResult{MI355_OK, d.scores[i], {0, 0}};
    } else {
      const uint64_t *h = (const uint64_t *)d.block.h;
      *o = CmpResult{MI355_OK, mi355_videocompare_distance(MI355_HASH_BLOCKHASH, h[i], h[d.n + i]), {h[i], h[d.n + i]}};
    }
  }
  static void failed(const CmpPair &, int rc, CmpResult *o) { *o = CmpResult{rc, 0.0, {0, 0}}; }
  static int status(const CmpResult &o) { return o.status; }
  void destroy() {
    free_lanes();
    blocks.destroy();
  }
};

// ---- the protocol, once. Every method runs with g->mu held.
template <class Kind>
struct SetQueue {
  using Item = QItem<typename Kind::Payload>;
  using Result = typename Kind::Result;
  using Payload = typename Kind::Payload;
  struct Set {
    uint64_t seq;  // launch order: set n of a lane is done => every earlier set of that lane is
    std::vector<uint64_t> tickets;
    int lane;      // which of the kind's streams carries it
    hipEvent_t done;
    int waiters;
    typename Kind::SetData data;
    bool collected = false;
  };
  // where a ticket stands: still pending (its payload), in a set in flight (the set and its index there), or collected (its result)
  struct Standing { const Payload *pending = nullptr; const Set *set = nullptr; size_t index = 0; const Result *result = nullptr; };
  static_assert(Kind::kLanesMax <= 32, "retire_done keeps the lanes in a mask");
  Kind kind;                     // the queue's own streams, scratch and blocks: made at the first submit (Kind::ensure)
  std::vector<Item> pending;
  std::deque<Set> sets;          // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> where;   // ticket -> seq
  std::unordered_map<uint64_t, Result> results;   // finished (or failed), not yet collected by the queue's wait entry
  uint64_t next_seq = 1;
  uint64_t n_items = 0, n_sets = 0, n_largest = 0, n_launches = 0;
  int expected = 0;              // rendezvous: a waiter lingers until this many items are pending ...
  unsigned linger_us = 0;        // ... or this long
  std::condition_variable cv;    // "a set has been launched"

  bool is_pending(uint64_t ticket) const {
    for (const Item &d : pending)
      if (d.ticket == ticket) return true;
    return false;
  }

  // is `ticket` an item of this queue that has not been collected?
  bool owns(uint64_t ticket) const { return where.count(ticket) || results.count(ticket) || is_pending(ticket); }

  // for an entry point that has to know something of the item before a refusal that must leave it collectable
  Standing find(uint64_t ticket) const {
    Standing st;
    for (const Item &d : pending)
      if (d.ticket == ticket) st.pending = &d.p;
    auto w = where.find(ticket);
    if (w != where.end())
      for (const Set &s : sets)
        if (s.seq == w->second)
          for (size_t i = 0; i < s.tickets.size(); i++)
            if (s.tickets[i] == ticket) { st.set = &s; st.index = i; }
    auto r = results.find(ticket);
    if (r != results.end()) st.result = &r->second;
    return st;
  }

  // what an entry point that serves another queue says to a ticket this queue owns
  static std::string foreign_refusal() { return std::string("group: a ") + Kind::kItem + "'s ticket (" + Kind::kWaitEntry + " collects it)"; }

  // a finished set: its results into `results` (once); nothing reads its pinned block afterwards, so the block is free again
  void collect(Set &s) {
    if (s.collected) return;
    s.collected = true;
    if (results.size() > 65536) results.clear();   // (results nobody ever collected)
    for (size_t i = 0; i < s.tickets.size(); i++) {
      kind.result(s.data, i, &results[s.tickets[i]]);
      where.erase(s.tickets[i]);
    }
    kind.blocks.give(&s.data.block);
  }

  // collected sets nobody waits inside leave: the event goes back to the free list
  void retire(GroupCore *g) {
    for (auto it = sets.begin(); it != sets.end();) {
      if (it->collected && it->waiters == 0) {
        g->events.push_back(it->done);
        it = sets.erase(it);
      } else {
        ++it;
      }
    }
  }

  // finished sets are collected without a waiter (a lane's stream is in order: its first unfinished set ends the search there;
  // the lanes finish independently)
  void retire_done(GroupCore *g) {
    unsigned unfinished = 0;   // lanes, as bits
    for (Set &s : sets) {
      if (s.collected || (unfinished >> s.lane & 1u)) continue;
      if (hipEventQuery(s.done) != hipSuccess) { (void)hipGetLastError(); unfinished |= 1u << s.lane; continue; }
      collect(s);
    }
    retire(g);
  }

  // Launches the pending items (all of them, or up to the set that carries `until`). A take is, in submission order, the items of
  // the front item's class, up to kSetMax; what it passes over keeps its order. The kind deals the take out as parts, each a set
  // on its lane's stream, behind the `ready` events of its own items only. A part that fails is told to each ticket it carried,
  // once, through `results`; the flush goes on and returns the first failure. The stats count per take, and what stood.
  int flush_locked(GroupCore *g, uint64_t until = 0) {
    bool reached = false;
    int first_rc = MI355_OK;
    while (!pending.empty() && !reached) {
      std::vector<Item> all, keep;
      for (Item &d : pending) {
        if (all.empty() || ((int)all.size() < Kind::kSetMax && Kind::same_class(all.front().p, d.p))) all.push_back(std::move(d));
        else keep.push_back(std::move(d));
      }
      pending.swap(keep);
      Part parts[Kind::kLanesMax];
      const int n_parts = kind.split(all, parts);
      size_t stood = 0;
      for (int k = 0; k < n_parts; k++) {
        const Item *take = all.data() + parts[k].begin;
        const size_t n = parts[k].end - parts[k].begin;
        const int lane = parts[k].lane;
        const hipStream_t stream = kind.lane_stream(lane);
        int launches = 0;
        std::string err;
        typename Kind::Plan plan;
        typename Kind::SetData data;
        int rc = kind.plan(take, n, &plan, &err);
        hipEvent_t done = take_event(g);
        if (!rc) {
          const size_t bytes = kind.block_bytes(plan);   // (0: this set has nothing to copy back)
          if (bytes && kind.blocks.free.empty()) retire_done(g);   // (a finished set nobody has collected gives its block back)
          if ((bytes && !kind.blocks.take(bytes, &data.block)) || !done) { rc = MI355_ERR_HIP; err = std::string("group: no event or pinned block for a ") + Kind::kName + " set"; }
        }
        for (size_t i = 0; i < n; i++)
          if (!rc && take[i].ready && hipStreamWaitEvent(stream, take[i].ready, 0) != hipSuccess) { rc = MI355_ERR_HIP; err = std::string("hipStreamWaitEvent(") + Kind::kItem + ")"; }
        if (!rc) rc = kind.launch(lane, plan, n, &data, &launches, &err);
        if (!rc && hipEventRecord(done, stream) != hipSuccess) { rc = MI355_ERR_HIP; err = std::string("hipEventRecord(") + Kind::kName + " set)"; }
        for (size_t i = 0; i < n; i++)
          if (take[i].ready) g->events.push_back(take[i].ready);
        if (rc) {
          (void)hipGetLastError();
          if (done) g->events.push_back(done);
          if (data.block.h) {
            // what did go out may still write the block: it is free again only behind the lane's stream
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
            kind.blocks.give(&data.block);
          }
          g->last_error = std::string("group: ") + Kind::kName + " launch failed: " + err;
          if (results.size() > 65536) results.clear();
          for (size_t i = 0; i < n; i++) Kind::failed(take[i].p, rc, &results[take[i].ticket]);   // told to the item's own wait, once
          if (!first_rc) first_rc = rc;
          continue;
        }
        kind.launched(g, plan, n);
        Set s{next_seq++, {}, lane, done, 0, std::move(data)};
        for (size_t i = 0; i < n; i++) { s.tickets.push_back(take[i].ticket); where[take[i].ticket] = s.seq; reached |= until != 0 && take[i].ticket == until; }
        sets.push_back(std::move(s));
        stood += n;
        n_launches += (uint64_t)launches;
      }
      if (!stood) continue;
      n_items += stood;
      n_sets++;
      if (stood > n_largest) n_largest = stood;
    }
    cv.notify_all();
    return first_rc;
  }

  // host wait for the set of `ticket`, and with it - its lane's stream being in order - for every earlier one of that lane; `lk`
  // owns g->mu on entry and on return, not while waiting
  int wait_unlocking(GroupCore *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
    auto it = where.find(ticket);
    if (it == where.end()) return MI355_OK;  // collected already (or failed: `results` has it)
    const uint64_t seq = it->second;
    const Waited w = wait_seq_unlocking(sets, seq, lk);
    if (w == Waited::kNothing) return MI355_OK;
    if (w == Waited::kFailed) return fail(g, MI355_ERR_HIP, std::string("hipEventSynchronize(group ") + Kind::kName + " set)");
    // (the set itself is still here: none retires while somebody waits inside it, and the lock has been held since)
    int lane = -1;
    for (const Set &s : sets)
      if (s.seq == seq) lane = s.lane;
    for (Set &s : sets)
      if (s.lane == lane && s.seq <= seq) collect(s);
    retire(g);
    return MI355_OK;
  }

  // waits for every set launched so far: for each lane's last uncollected one (their results stay collectable)
  int wait_all_unlocking(GroupCore *g, std::unique_lock<std::mutex> &lk) {
    uint64_t last[Kind::kLanesMax] = {0};
    for (const Set &s : sets)
      if (!s.collected) last[s.lane] = s.tickets.front();
    for (uint64_t t : last)
      if (t)
        if (int rc = wait_unlocking(g, lk, t)) return rc;
    return MI355_OK;
  }

  void set_rendezvous(int expected_streams, unsigned linger) {
    expected = expected_streams;
    linger_us = linger;
  }

  // the tail of a submit, behind the entry point's own checks of the payload; want_ready: false for an item nothing will read
  int submit(GroupCore *g, mi355_ctx *ctx, const typename Kind::Payload &p, bool want_ready, uint64_t *ticket) {
    if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
    if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
    if (int rc = kind.ensure(g)) return rc;
    retire_done(g);
    Item d{p, 0, nullptr};
    if (want_ready)
      if (int rc = record_ready(g, ctx, &d.ready)) return rc;
    d.ticket = g->next_ticket++;
    *ticket = d.ticket;
    pending.push_back(d);
    // everybody is here (rendezvous), or a launch set is full: go. The item has been accepted whatever that launch does (a failure
    // is told to the waits of the items it carried).
    const int full = expected > 0 && expected < Kind::kSetMax ? expected : Kind::kSetMax;
    if ((int)pending.size() >= full) (void)flush_locked(g);
    return MI355_OK;
  }

  // the body of a wait: *out is the item's result, taken out of `results` - once
  int wait(GroupCore *g, std::unique_lock<std::mutex> &lk, uint64_t ticket, Result *out) {
    // another queue's, a collected or an unknown ticket: refused before anything is launched or waited for
    if (!owns(ticket)) return fail(g, MI355_ERR_INVALID_ARG, std::string("group: not the ticket of a ") + Kind::kItem + " that is still to be collected");
    if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
    if (is_pending(ticket)) {
      // rendezvous: the other instances of this interval are about to submit - linger for them (bounded), then launch what is there
      if (expected > 0 && linger_us > 0) {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(linger_us);
        while (is_pending(ticket) && (int)pending.size() < expected) {
          if (cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
        }
      }
      if (is_pending(ticket)) (void)flush_locked(g, ticket);   // (a failure of this item's own launch is in `results`)
    }
    if (int rc = wait_unlocking(g, lk, ticket)) return rc;
    auto r = results.find(ticket);
    if (r == results.end()) return fail(g, MI355_ERR_INVALID_ARG, std::string("group: this ") + Kind::kItem + "'s result has been collected already");   // (by a concurrent wait)
    *out = std::move(r->second);
    results.erase(r);
    if (const int status = Kind::status(*out)) return fail(g, status, std::string("group: the launch that carried this ") + Kind::kItem + " failed");
    return MI355_OK;
  }

  void stats(uint64_t out[4]) const {
    out[0] = n_items;
    out[1] = n_sets;
    out[2] = n_largest;
    out[3] = n_launches;
  }

  // The queue's part of mi355_group_destroy (takes g->mu itself): items still pending are launched and waited for - their buffers
  // belong to callers who may free them once destroy returns, and a detector's destination is complete by then.
  void destroy(GroupCore *g) {
    if (!kind.lane_stream(0)) return;
    if (kind.set_up()) {
      std::lock_guard<std::mutex> lk(g->mu);
      (void)flush_locked(g);
    }
    for (int l = 0; l < kind.lanes(); l++) (void)hipStreamSynchronize(kind.lane_stream(l));
    for (Set &s : sets) {
      (void)hipEventDestroy(s.done);
      kind.blocks.give(&s.data.block);
    }
    sets.clear();
    for (Item &d : pending)
      if (d.ready) (void)hipEventDestroy(d.ready);
    pending.clear();
    kind.destroy();
  }
};

}  // namespace

struct mi355_group : GroupCore {
  int max_batch = 8;
  hipStream_t stream = nullptr;
  std::vector<Desc> pending;
  std::deque<Batch> batches;       // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> where;  // ticket -> seq of its batch, for launched batches not yet retired
  std::unordered_map<uint64_t, int> failed;      // ticket -> status of the launch that did not happen (reported by wait / order_after)
  uint64_t next_seq = 1;
  uint64_t n_frames = 0, n_batched_launch_pairs = 0, n_single = 0;
  // table references of retired batches: dropping the last reference to a table frees 64 MiB behind a device-wide wait, which
  // does not belong under `mu` - the entry points empty this list into a local one that dies after they have unlocked (Locked)
  std::vector<std::shared_ptr<void>> dead_refs;
  // ---- the seven set queues: each its own streams (and scratch, and blocks), created at its first submit, independent of the
  // filter batches above and of each other
  SetQueue<CmpKind> cmp; // videocompare pairs (Dssim / Blockhash)
  SetQueue<CdKind> cd;   // colordetect frames
  SetQueue<HdKind> hd;   // hsvdetector frames
  SetQueue<YdKind> yd;   // decoder tensors
  SetQueue<HnKind> hn;   // hand tensors (palm and landmarks)
  SetQueue<HfKind> hf;   // hsvfilter frames (in place)
  SetQueue<ClKind> cl;   // colorlut frames (each with its context's LUT)
};

namespace {

// g->mu for the scope, and behind it the table references the scope retired (destroyed last, i.e. outside the lock)
struct Locked {
  std::vector<std::shared_ptr<void>> reap;
  mi355_group *g;
  std::unique_lock<std::mutex> lk;
  explicit Locked(mi355_group *g_) : g(g_), lk(g_->mu) {}
  ~Locked() {
    if (!lk.owns_lock()) lk.lock();
    reap.swap(g->dead_refs);
    lk.unlock();
  }
};

void retire_front(mi355_group *g) {
  Batch &b = g->batches.front();
  for (uint64_t t : b.tickets) g->where.erase(t);
  g->events.push_back(b.done);
  if (b.table_ref) g->dead_refs.push_back(std::move(b.table_ref));
  g->batches.pop_front();
}

// batches that have finished leave without anybody waiting for them (a stream that only ever orders its own stream behind its
// frames never waits here; its batches, and the table references they hold, must not pile up)
void retire_done(mi355_group *g) {
  while (!g->batches.empty() && g->batches.front().waiters == 0) {
    if (hipEventQuery(g->batches.front().done) != hipSuccess) { (void)hipGetLastError(); break; }
    retire_front(g);
  }
}

bool same_class(const Desc &a, const Desc &b) {
  return a.batchable && b.batchable && a.fused == b.fused && a.width == b.width && a.height == b.height && a.stride == b.stride && a.format == b.format && a.table == b.table &&
         std::memcmp(&a.hs, &b.hs, sizeof(a.hs)) == 0 && a.ctx->force_generic == b.ctx->force_generic && (a.ctx->hsv_nt == 2) == (b.ctx->hsv_nt == 2);
}

// launches what is pending, batch by batch - all of it, or (until != 0) only up to the batch that carries ticket `until`: what a
// waiter needs; the frames behind it stay and meet the other streams' next frames in a fuller batch. g->mu held.
int flush_locked(mi355_group *g, uint64_t until = 0) {
  bool reached = false;
  while (!g->pending.empty() && !reached) {
    std::vector<Desc> take, keep;
    std::vector<mi355_ctx *> blocked;  // streams with a frame left behind: their later frames must not overtake it
    const Desc first = g->pending.front();
    for (const Desc &d : g->pending) {
      bool stream_blocked = false;
      for (mi355_ctx *c : blocked) stream_blocked |= c == d.ctx;
      const bool fits = take.empty() || (!stream_blocked && (int)take.size() < g->max_batch && same_class(first, d));
      if (fits) take.push_back(d);
      else keep.push_back(d);
      // ONE frame per stream and batch: the hsvfilter launch of a batch runs over all its frames before the colorlut launch
      // does, so a frame that reads what the stream's previous frame wrote (or simply comes after it) belongs to a later batch
      if (!stream_blocked) blocked.push_back(d.ctx);
    }
    g->pending.swap(keep);
    PixFmt fmt;
    (void)pixfmt_of(first.format, &fmt);
    hipEvent_t done = take_event(g);
    if (!done) return fail(g, MI355_ERR_HIP, "hipEventCreate");
    int rc = MI355_OK;
    if (first.batchable) {
      uint8_t *srcs[kMultiFrames], *dsts[kMultiFrames];
      for (size_t i = 0; i < take.size(); i++) {
        srcs[i] = take[i].src;
        dsts[i] = take[i].dst;
        if (take[i].ready && hipStreamWaitEvent(g->stream, take[i].ready, 0) != hipSuccess) rc = MI355_ERR_HIP;
      }
      // (fused: `table` is the composed hsvfilter -> colorlut table of these settings: the gather IS the chain, one launch)
      if (!rc && !first.fused) rc = launch_hsvfilter_multi(first.ctx, g->stream, srcs, (int)take.size(), first.width, first.height, fmt, first.hs);
      if (!rc) rc = launch_colorlut_multi(first.ctx, g->stream, first.table, srcs, dsts, (int)take.size(), first.width, first.height, first.fused);
      if (!rc && hipEventRecord(done, g->stream) != hipSuccess) rc = MI355_ERR_HIP;
      g->n_batched_launch_pairs++;
    } else {
      // not the batched kernels' geometry: this frame through its context's own path, on its own stream, after everything
      // launched so far (order), and the group's stream after it
      const Desc &d = take[0];
      const size_t pitch = (size_t)d.stride * (size_t)d.height;
      if (!g->batches.empty() && hipStreamWaitEvent(d.ctx->stream, g->batches.back().done, 0) != hipSuccess) rc = MI355_ERR_HIP;
      if (!rc && d.fused) rc = launch_hsv_colorlut(d.ctx, d.src, pitch, d.stride, d.dst, pitch, d.stride, 1, d.width, d.height, d.hs);
      if (!rc && !d.fused) rc = launch_hsvfilter(d.ctx, d.src, 1, pitch, d.width, d.height, d.stride, fmt, d.hs);
      if (!rc && !d.fused) rc = launch_colorlut(d.ctx, d.src, pitch, d.stride, d.dst, pitch, d.stride, 1, d.width, d.height, d.format);
      if (!rc && hipEventRecord(done, d.ctx->stream) != hipSuccess) rc = MI355_ERR_HIP;
      if (!rc && hipStreamWaitEvent(g->stream, done, 0) != hipSuccess) rc = MI355_ERR_HIP;
      if (rc && rc != MI355_ERR_HIP) g->last_error = d.ctx->last_error;
      g->n_single++;
    }
    for (const Desc &d : take)
      if (d.ready) g->events.push_back(d.ready);
    if (rc) {
      // the frames of this batch have left `pending` and will never be in `where`: whoever waits for one of them is told
      (void)hipGetLastError();
      g->events.push_back(done);
      if (g->failed.size() > 65536) g->failed.clear();  // (tickets nobody ever waited for)
      for (const Desc &d : take) g->failed[d.ticket] = rc;
      if (g->last_error.empty()) g->last_error = "group launch failed";
      return rc;
    }
    Batch b{g->next_seq++, {}, done, 0, first.batchable ? first.table_ref : std::shared_ptr<void>()};
    for (const Desc &d : take) { b.tickets.push_back(d.ticket); g->where[d.ticket] = b.seq; reached |= until != 0 && d.ticket == until; }
    g->batches.push_back(std::move(b));
    g->n_frames += take.size();
  }
  return MI355_OK;
}

// Waits (on the host) for the batch that holds `ticket` - and with it, the stream being in order, for every earlier one. The
// lock is NOT held while waiting: other streams' threads keep submitting. `lk` owns g->mu on entry and on return.
int wait_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
  auto bad = g->failed.find(ticket);
  if (bad != g->failed.end()) {
    const int rc = bad->second;
    g->failed.erase(bad);
    return fail(g, rc, "group: the launch that carried this frame failed");
  }
  auto it = g->where.find(ticket);
  if (it == g->where.end()) return MI355_OK;  // launched and already retired (by this or another waiter)
  const uint64_t seq = it->second;
  const Waited w = wait_seq_unlocking(g->batches, seq, lk);
  if (w == Waited::kNothing) return MI355_OK;
  if (w == Waited::kFailed) return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group batch)");
  // everything up to that batch is done: retire from the front (batches somebody still waits in stay until they leave)
  while (!g->batches.empty() && g->batches.front().seq <= seq && g->batches.front().waiters == 0) retire_front(g);
  return MI355_OK;
}

// waits for everything launched so far
int wait_all_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk) {
  while (!g->batches.empty()) {
    const uint64_t t = g->batches.back().tickets.back();
    const size_t before = g->batches.size();
    int rc = wait_unlocking(g, lk, t);
    if (rc) return rc;
    if (!g->batches.empty() && g->batches.size() >= before && g->batches.back().tickets.back() == t) break;  // held by other waiters: done anyway
  }
  return MI355_OK;
}

// ------------------------------------------------------------------ the set queues, where an entry point names them all

// f(queue) for each set queue but the compare queue, in the order every walk goes through them. This is what wait_all and the
// foreign-ticket refusal below reach: wait_all does not wait for pairs, and no other entry refuses a pair's ticket by name - the
// one difference between the compare queue and the others here.
template <class F>
void for_each_queue_but_compare(mi355_group *g, F &&f) {
  f(g->cd);
  f(g->hd);
  f(g->yd);
  f(g->hn);
  f(g->hf);
  f(g->cl);
}

// ... and for all seven, the compare queue first: flush and destroy treat it as every other
template <class F>
void for_each_set_queue(mi355_group *g, F &&f) {
  f(g->cmp);
  for_each_queue_but_compare(g, f);
}

// A set queue's ticket presented to an entry point that serves another queue: refused (non-zero), and left collectable.
int refuse_set_queue_ticket(mi355_group *g, uint64_t ticket) {
  std::string owner;
  for_each_queue_but_compare(g, [&](auto &q) {
    if (owner.empty() && q.owns(ticket)) owner = q.foreign_refusal();
  });
  return owner.empty() ? MI355_OK : fail(g, MI355_ERR_INVALID_ARG, owner);
}

// ---- the bodies the set queues' entry points share; `q` names the queue (a null group has none to take the address of)

template <class Q>
int queue_set_rendezvous(mi355_group *g, Q mi355_group::*q, int expected_streams, unsigned linger_us) {
  if (!g || expected_streams < 0) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  (g->*q).set_rendezvous(expected_streams, linger_us);
  return MI355_OK;
}

// {items launched, launch sets, items in the largest set, kernel launches}: the first `columns` of them
template <class Q>
int queue_stats(mi355_group *g, Q mi355_group::*q, uint64_t *stats, int columns = 4) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  uint64_t all[4];
  (g->*q).stats(all);
  std::copy(all, all + columns, stats);
  return MI355_OK;
}

// the wait of a kind whose result is the launch's status alone (FrameKind)
template <class Q>
int queue_wait_status(mi355_group *g, Q mi355_group::*q, uint64_t ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  int status = MI355_OK;
  return (g->*q).wait(g, L.lk, ticket, &status);
}

}  // namespace

extern "C" {

mi355_group *mi355_group_create(int device, int max_batch, int *status) {
  if (max_batch < 0 || max_batch > kMultiFrames) { if (status) *status = MI355_ERR_INVALID_ARG; return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); if (status) *status = MI355_ERR_NO_DEVICE; return nullptr; }
  mi355_group *g = new mi355_group();
  g->device = device;
  g->max_batch = max_batch ? max_batch : 8;  // eight 4K frames: what one launch should hold to stay inside the Infinity Cache
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    delete g;
    if (status) *status = MI355_ERR_HIP;
    return nullptr;
  }
  if (status) *status = MI355_OK;
  return g;
}

void mi355_group_destroy(mi355_group *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  {
    Locked L(g);
    (void)flush_locked(g);
    (void)wait_all_unlocking(g, L.lk);
  }
  (void)hipStreamSynchronize(g->stream);
  for_each_set_queue(g, [&](auto &q) { q.destroy(g); });   // (a queue that was never set up has nothing: SetQueue::destroy)
  for (Batch &b : g->batches) (void)hipEventDestroy(b.done);   // (normally none left: wait_all retired them)
  for (Desc &d : g->pending)
    if (d.ready) (void)hipEventDestroy(d.ready);
  g->pending.clear();
  g->batches.clear();  // their table references go here, after the stream has drained
  g->dead_refs.clear();
  for (hipEvent_t e : g->events) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(g->stream);
  delete g;
}

const char *mi355_group_last_error(mi355_group *g) { return g ? g->last_error.c_str() : "null group"; }

static int submit_frame(mi355_group *g, mi355_ctx *ctx, uint8_t *d_src, uint8_t *d_dst, int width, int height, int stride, int format,
                        const mi355_hsv_settings *settings, uint64_t *ticket, bool fused) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  PixFmt fmt;
  if (!ctx || !d_src || !d_dst || !settings || width <= 0 || height <= 0 || !pixfmt_of(format, &fmt) || (size_t)stride < (size_t)width * fmt.pixel_stride)
    return fail(g, MI355_ERR_INVALID_ARG, "group: bad frame");
  // the chain exists for the one format both elements accept (hsvfilter/imp.rs:252-266, colorlut/imp.rs:125-137): refused here,
  // not as a failed launch of a whole batch later
  if (format != MI355_FMT_RGBA) return fail(g, MI355_ERR_INVALID_ARG, "group: hsvfilter ! colorlut takes RGBA frames only");
  if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
  if (!ctx->lut.loaded) return fail(g, MI355_ERR_NOT_CONFIGURED, "No LUT configured");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  Desc d{};
  d.ctx = ctx; d.src = d_src; d.dst = d_dst; d.width = width; d.height = height; d.stride = stride; d.format = format; d.hs = *settings;
  d.fused = fused;
  retire_done(g);
  // a composed table is 64 MiB built by two launches over 2^24 colours: worth it for settings that stay (the fused entry point
  // has the same rule: eight calls), not for a hue shift animated frame by frame - those frames take their context's own path
  bool settled = true;
  if (fused) {
    if (std::memcmp(&ctx->group_fused_hs, settings, sizeof(*settings)) == 0) { if (ctx->group_fused_stable < 1000000u) ctx->group_fused_stable++; }
    else { ctx->group_fused_hs = *settings; ctx->group_fused_stable = 1; }
    settled = ctx->group_fused_stable >= 8u;
  }
  const uint8_t *one[1] = {d_src};
  // (the two-launch form filters d_src in place and then reads it: not onto itself; the fused form reads a tile and writes the same tile)
  d.batchable = settled && format == MI355_FMT_RGBA && (fused || d_src != d_dst) && hsvfilter_multi_applicable(one, 1, width, height, stride, fmt) && width % 4 == 0 &&
                width >= 128 && (uintptr_t)d_dst % 16 == 0 && ctx->lut_variant == 0 && ctx->hsv_table_mode != 2 && (!fused || ctx->lut.is3d);
  if (d.batchable && (fused ? colorlut_multi_fused_table(ctx, settings, &d.table) : colorlut_multi_table(ctx, &d.table)) != MI355_OK) {  // (the build, if any, is on ctx->stream: before `ready`)
    (void)hipGetLastError();
    d.batchable = false;
    d.table = nullptr;
  }
  // (this thread is the one that drives ctx, and the reference is copied from ctx's own: the registry's "sole user" test cannot
  // run concurrently with this copy)
  if (d.batchable) d.table_ref = ctx->lut.table_ref[fused ? 1 : 0];
  // the frame starts after what ctx's stream holds now (an upload, the table build)
  if (int rc = record_ready(g, ctx, &d.ready)) return rc;
  d.ticket = g->next_ticket++;
  if (ticket) *ticket = d.ticket;
  g->pending.push_back(d);
  // enough for a full launch: the batch of the oldest pending frame goes now (the rest keeps collecting). This frame has been
  // accepted whatever that launch does: a failed batch is reported to the frames it carried (g->failed: their wait / order_after),
  // which may or may not include this one - never as a refusal of this submit, whose caller would then reuse buffers the group
  // still refers to.
  if ((int)g->pending.size() >= g->max_batch) (void)flush_locked(g, g->pending.front().ticket);
  return MI355_OK;
}

int mi355_group_submit_chain(mi355_group *g, mi355_ctx *ctx, uint8_t *d_src, uint8_t *d_dst, int width, int height, int stride, int format,
                             const mi355_hsv_settings *settings, uint64_t *ticket) {
  return submit_frame(g, ctx, d_src, d_dst, width, height, stride, format, settings, ticket, false);
}

int mi355_group_submit_fused(mi355_group *g, mi355_ctx *ctx, uint8_t *d_src, uint8_t *d_dst, int width, int height, int stride, int format,
                             const mi355_hsv_settings *settings, uint64_t *ticket) {
  return submit_frame(g, ctx, d_src, d_dst, width, height, stride, format, settings, ticket, true);
}

int mi355_group_flush(mi355_group *g) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  int first = flush_locked(g);
  for_each_set_queue(g, [&](auto &q) {   // every queue that has been set up is launched; the first failure is the answer
    const int r = q.kind.set_up() ? q.flush_locked(g) : MI355_OK;
    if (!first) first = r;
  });
  return first;
}

// ---------------------------------------------------------------- videocompare pairs (Dssim / Blockhash) of independent elements

int mi355_group_set_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::cmp, expected_streams, linger_us);
}

int mi355_group_set_compare_lanes(mi355_group *g, int lanes) {
  if (!g || lanes < 1 || lanes > kCmpMaxLanes) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (g->cmp.kind.set_up()) return fail(g, MI355_ERR_INVALID_ARG, "group: the compare queue's streams exist already (set the lanes before the first submit_compare)");
  g->cmp.kind.n_lanes = lanes;
  return MI355_OK;
}

int mi355_group_submit_compare(mi355_group *g, mi355_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_frame, int stride, int width, int height, int format,
                               int algo, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  PixFmt fmt;
  if (!ctx || !d_ref || !d_frame || width <= 0 || height <= 0 || !pixfmt_of(format, &fmt) || (format != MI355_FMT_RGB && format != MI355_FMT_RGBA) ||
      (size_t)stride < (size_t)width * fmt.pixel_stride)
    return fail(g, MI355_ERR_INVALID_ARG, "group: bad frame pair (videocompare's engines take packed RGB / RGBA)");
  if (algo != MI355_HASH_DSSIM && algo != MI355_HASH_BLOCKHASH)
    return fail(g, MI355_ERR_UNSUPPORTED, "group: pairs are batched for hash-algorithm dssim and blockhash; the resize hashes go through their context");
  if (algo == MI355_HASH_BLOCKHASH && (width % 8 != 0 || height % 8 != 0))
    return fail(g, MI355_ERR_UNSUPPORTED, "group: blockhash batches take frames of 8 x 8 whole blocks (the any-size path goes through its context)");
  // the pair starts after what the stream's own context holds now (an upload); a caller may leave the ticket to flush
  uint64_t t = 0;
  const int rc = g->cmp.submit(g, ctx, CmpPair{d_ref, d_frame, width, height, stride, format, algo, ctx->dssim_translucent, ctx->dssim_fast}, true, &t);
  if (!rc && ticket) *ticket = t;
  return rc;
}

int mi355_group_wait_compare(mi355_group *g, uint64_t ticket, double *distance, uint64_t hashes[2]) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  CmpResult res;
  if (int rc = g->cmp.wait(g, L.lk, ticket, &res)) return rc;
  if (distance) *distance = res.distance;
  if (hashes) { hashes[0] = res.hashes[0]; hashes[1] = res.hashes[1]; }
  return MI355_OK;
}

// (the compare queue reports no launch column)
int mi355_group_compare_stats(mi355_group *g, uint64_t stats[3]) { return queue_stats(g, &mi355_group::cmp, stats, 3); }

// ---------------------------------------------------------------- the set queues' entry points: each checks its own arguments and
// hands over to SetQueue<Kind> (submit's tail, the body of wait, stats)

int mi355_group_set_colordetect_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::cd, expected_streams, linger_us);
}

int mi355_group_submit_colordetect(mi355_group *g, mi355_ctx *ctx, const uint8_t *d_data, size_t data_len, int format, int quality, int max_colors,
                                   uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context or ticket");
  const char *why = nullptr;
  int rc = colordetect_check_frame(data_len, format, quality, max_colors, &why);
  if (rc) return fail(g, rc, why);
  if (data_len && !d_data) return fail(g, MI355_ERR_INVALID_ARG, "colordetect: null frame");
  return g->cd.submit(g, ctx, CdFrame{d_data, data_len, format, quality, max_colors}, true, ticket);
}

int mi355_group_wait_colordetect(mi355_group *g, uint64_t ticket, uint8_t palette_rgb[255 * 3], int *n_colors) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!palette_rgb || !n_colors) return fail(g, MI355_ERR_INVALID_ARG, "group: null result arrays");
  CdOut res;
  if (int rc = g->cd.wait(g, L.lk, ticket, &res)) return rc;
  std::memcpy(palette_rgb, res.rgb, sizeof(res.rgb));
  *n_colors = res.n_colors;
  return MI355_OK;
}

int mi355_group_colordetect_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::cd, stats); }

int mi355_group_set_hsvdetect_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::hd, expected_streams, linger_us);
}

int mi355_group_submit_hsvdetect(mi355_group *g, mi355_ctx *ctx, const uint8_t *d_src, int src_stride, int src_format, uint8_t *d_dst, int dst_stride,
                                 int dst_format, int width, int height, const mi355_hsvdetect_settings *settings, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context or ticket");
  HdFrame f{};
  const char *why = nullptr;
  int rc = hsvdetect_check_frames(d_src, src_stride, src_format, d_dst, dst_stride, dst_format, 1, width, height, settings, &f.sfmt, &f.dst_alpha_first,
                                  &f.dst_bgr, &why);
  if (rc) return fail(g, rc, why);
  f.src = d_src;
  f.dst = d_dst;
  f.src_stride = src_stride;
  f.dst_stride = dst_stride;
  f.width = width;
  f.height = height;
  f.s = *settings;
  f.force_generic = ctx->force_generic;
  // an empty frame reads nothing: it does not make the set wait for its stream
  return g->hd.submit(g, ctx, f, width > 0 && height > 0, ticket);
}

int mi355_group_wait_hsvdetect(mi355_group *g, uint64_t ticket) { return queue_wait_status(g, &mi355_group::hd, ticket); }

int mi355_group_hsvdetect_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::hd, stats); }

int mi355_selftest_hsvdetect_plan(int n_cu, int blocks_per_cu, unsigned units_per_block, int n_jobs, const uint64_t *units, uint32_t *first_block,
                                  uint32_t *blocks, uint32_t *total_blocks) {
  return hsvdetect_plan(n_cu, blocks_per_cu, units_per_block, n_jobs, units, first_block, blocks, total_blocks);
}

int mi355_group_set_hsvfilter_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::hf, expected_streams, linger_us);
}

int mi355_group_submit_hsvfilter(mi355_group *g, mi355_ctx *ctx, uint8_t *d_data, int width, int height, int stride, int format,
                                 const mi355_hsv_settings *settings, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context or ticket");
  HfFrame f{};
  const char *why = nullptr;
  if (int rc = hsvfilter_check_frames(d_data, 1, 0, width, height, stride, format, settings, &f.fmt, &why)) return fail(g, rc, why);
  f.data = d_data;
  f.width = width;
  f.height = height;
  f.stride = stride;
  f.s = *settings;
  f.force_generic = ctx->force_generic;
  f.hsv_nt = ctx->hsv_nt;
  // In place: a frame that shares bytes with a pending one must not share its launch. What is pending goes out first (sets of the
  // queue's one stream run in order), so the two come out as if filtered one after the other. A failure of that launch is told to
  // the waits of the frames it carried; this frame is queued whatever it did.
  bool meets = false;
  for (const auto &d : g->hf.pending) meets |= hsvfilter_frames_overlap(d.p, f);
  if (meets) {
    if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
    (void)g->hf.flush_locked(g);
  }
  // an empty frame touches nothing: it does not make the set wait for its stream
  return g->hf.submit(g, ctx, f, width > 0 && height > 0, ticket);
}

int mi355_group_wait_hsvfilter(mi355_group *g, uint64_t ticket) { return queue_wait_status(g, &mi355_group::hf, ticket); }

int mi355_group_hsvfilter_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::hf, stats); }

int mi355_selftest_hsvfilter_set_plan(int n_cu, const mi355_hsvfilter_plan_frame *frames, int n_frames, mi355_hsvfilter_plan_out *out, int *n_sets) {
  if (n_cu < 1 || n_frames < 0 || !n_sets || (n_frames && (!frames || !out))) return MI355_ERR_INVALID_ARG;
  std::vector<HfFrame> fr((size_t)n_frames);
  for (int i = 0; i < n_frames; i++) {
    const mi355_hsvfilter_plan_frame &p = frames[i];
    HfFrame &f = fr[(size_t)i];
    const char *why = nullptr;
    // (a frame with a pixel has an address: null is what submit refuses, any other number is as good as another)
    if (hsvfilter_check_frames((const uint8_t *)(uintptr_t)p.address, 1, 0, p.width, p.height, p.stride, p.format, &p.settings, &f.fmt, &why)) return MI355_ERR_INVALID_ARG;
    f.data = (uint8_t *)(uintptr_t)p.address;
    f.width = p.width;
    f.height = p.height;
    f.stride = p.stride;
    f.s = p.settings;
    f.force_generic = p.force_generic;
  }
  return hsvfilter_set_plan(n_cu, fr.data(), n_frames, out, n_sets);
}

// One frame as the colorlut queue takes it, for the submit entry and the selftest alike: the lone entry's checks (ctx.hip), then the
// queue's own - the element never works in place, so a frame whose own source and destination meet is refused.
static int colorlut_frame_of(bool lut_loaded, const uint8_t *d_src, int src_stride, uint8_t *d_dst, int dst_stride, int width, int height, int format,
                             ClFrame *f, const char **why) {
  int bpp = 0;
  if (int rc = colorlut_check_frames(lut_loaded, d_src, 0, src_stride, d_dst, 0, dst_stride, 1, width, height, format, &bpp, why)) return rc;
  *f = ClFrame{};
  f->src = d_src;
  f->dst = d_dst;
  f->src_stride = src_stride;
  f->dst_stride = dst_stride;
  f->width = width;
  f->height = height;
  f->format = format;
  f->size = 2;
  if (colorlut_frame_in_place(*f)) { *why = "colorlut: the frame's source and destination overlap"; return MI355_ERR_INVALID_ARG; }
  return MI355_OK;
}

int mi355_group_set_colorlut_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::cl, expected_streams, linger_us);
}

int mi355_group_submit_colorlut(mi355_group *g, mi355_ctx *ctx, const uint8_t *d_src, int src_stride, uint8_t *d_dst, int dst_stride, int width, int height,
                                int format, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context or ticket");
  ClFrame f{};
  const char *why = nullptr;
  if (int rc = colorlut_frame_of(ctx->lut.loaded, d_src, src_stride, d_dst, dst_stride, width, height, format, &f, &why)) return fail(g, rc, why);
  // the context's LUT, borrowed until the wait returns: the cells stay where mi355_colorlut_load put them
  const LutDevice &lut = ctx->lut;
  f.cells = lut.d_cells;
  f.is3d = lut.is3d;
  f.size = lut.size;
  for (int c = 0; c < 3; c++) { f.scale[c] = lut.scale[c]; f.offset[c] = lut.offset[c]; }
  f.force_generic = ctx->force_generic;
  // A frame that writes what a pending one reads or writes, or reads what a pending one writes, must not share its launch. What is
  // pending goes out first (sets of the queue's one stream run in order), so the frames come out as the lone calls in submission
  // order. A failure of that launch is told to the waits of the frames it carried; this frame is queued whatever it did.
  bool meets = false;
  for (const auto &d : g->cl.pending) meets |= colorlut_frames_meet(d.p, f);
  if (meets) {
    if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
    (void)g->cl.flush_locked(g);
  }
  // an empty frame touches nothing: it does not make the set wait for its stream
  return g->cl.submit(g, ctx, f, width > 0 && height > 0, ticket);
}

int mi355_group_wait_colorlut(mi355_group *g, uint64_t ticket) { return queue_wait_status(g, &mi355_group::cl, ticket); }

int mi355_group_colorlut_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::cl, stats); }

int mi355_selftest_colorlut_set_plan(int n_cu, const mi355_colorlut_plan_frame *frames, int n_frames, mi355_colorlut_plan_out *out, int *n_sets) {
  if (n_cu < 1 || n_frames < 0 || !n_sets || (n_frames && (!frames || !out))) return MI355_ERR_INVALID_ARG;
  std::vector<ClFrame> fr((size_t)n_frames);
  for (int i = 0; i < n_frames; i++) {
    const mi355_colorlut_plan_frame &p = frames[i];
    const char *why = nullptr;
    // (a LUT is taken as loaded - the plan does not depend on it; a frame with a pixel has addresses: null is what submit refuses)
    if (colorlut_frame_of(true, (const uint8_t *)(uintptr_t)p.src_address, p.src_stride, (uint8_t *)(uintptr_t)p.dst_address, p.dst_stride, p.width, p.height,
                          p.format, &fr[(size_t)i], &why))
      return MI355_ERR_INVALID_ARG;
    fr[(size_t)i].force_generic = p.force_generic;
  }
  return colorlut_set_plan(n_cu, fr.data(), n_frames, out, n_sets);
}

int mi355_group_set_yolodec_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::yd, expected_streams, linger_us);
}

int mi355_group_submit_yolodec(mi355_group *g, mi355_ctx *ctx, const float *d_tensor, int layout, uint32_t num_fields, uint32_t num_candidates,
                               const mi355_yolo_params *p, uint32_t max_dets, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !p || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context, settings or ticket");
  const char *why = nullptr;
  int rc = yolodec_check_args((size_t)num_fields * num_candidates * 4, 1, layout, num_fields, num_candidates, &why);
  if (rc) return fail(g, rc, why);
  if (num_candidates && (!d_tensor || (uintptr_t)d_tensor % 4 != 0)) return fail(g, MI355_ERR_INVALID_ARG, "yolodec: null or misaligned tensors");
  // a tensor without a candidate is not read: it does not make the set wait for its stream (the model's last kernel, an upload)
  return g->yd.submit(g, ctx, YdTensor{d_tensor, layout, num_fields, num_candidates, max_dets, *p, nullptr}, num_candidates != 0, ticket);
}

int mi355_group_submit_yolox_head(mi355_group *g, mi355_ctx *ctx, const mi355_yolox_level *levels, int n_levels, uint32_t num_classes, const mi355_yolo_params *p,
                                  uint32_t max_dets, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !p || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context, settings or ticket");
  const char *why = nullptr;
  uint32_t A = 0;
  int rc = yolox_head_check_shape(levels, n_levels, 1, num_classes, &A, &why);
  if (!rc) rc = yolox_head_check_maps(levels, n_levels, &why);
  if (rc) return fail(g, rc, why);
  // a member of the decoder queue as a tensor is: 5 + C fields, A candidates (at least one: the maps are always read)
  auto head = std::make_shared<YdHead>();
  for (int l = 0; l < n_levels; l++) head->lv[l] = levels[l];
  head->n_levels = n_levels;
  return g->yd.submit(g, ctx, YdTensor{nullptr, MI355_YOLO_X_HEAD, 5 + num_classes, A, max_dets, *p, std::move(head)}, true, ticket);
}

int mi355_group_submit_yolox_infer(mi355_group *g, mi355_ctx *ctx, mi355_yolox_net *net, const uint8_t *d_frame, size_t stride, uint32_t width, uint32_t height,
                                   const mi355_yolo_params *p, uint32_t max_dets, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !net || !p || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context, net, settings or ticket");
  // the lone call's checks for one frame, in its order; only what _finalize froze is read of the net
  const char *why = nullptr;
  if (const int rc = yolox_net_check_size(height, width, &why)) return fail(g, rc, why);
  YxNetInfo info;
  yolox_net_info(net, &info);
  if (!info.finalized) return fail(g, MI355_ERR_NOT_CONFIGURED, "yolox_net: inference before finalize");
  if (stride < (size_t)3 * width) return fail(g, MI355_ERR_INVALID_ARG, "yolox_input: stride below the row or frame pitch below the frame");
  if (!d_frame) return fail(g, MI355_ERR_INVALID_ARG, "yolox_input: null frames, or null or misaligned output");
  if (info.device != ctx->device) return fail(g, MI355_ERR_INVALID_ARG, "group: the net's context is on another device than the member's");
  // ... and its last: the head's shape checks of the three levels (a frame of more than 65536 candidates is refused there)
  mi355_yolox_level lv[3] = {};
  for (int l = 0; l < 3; l++) lv[l].h = height >> (3 + l), lv[l].w = width >> (3 + l), lv[l].stride = 8u << l;
  uint32_t A = 0;
  if (const int rc = yolox_head_check_shape(lv, 3, 1, info.num_classes, &A, &why)) return fail(g, rc, why);
  auto infer = std::make_shared<YdInfer>(YdInfer{net, info.serial, d_frame, stride, width, height});
  const int rc = g->yd.submit(g, ctx, YdTensor{nullptr, MI355_YOLO_X_INFER, 5 + info.num_classes, A, max_dets, *p, nullptr, std::move(infer)}, true, ticket);
  if (!rc) g->yd.kind.infer_tickets[*ticket] = info.serial;
  return rc;
}

int mi355_group_release_yolox_net(mi355_group *g, const mi355_yolox_net *net) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!net) return fail(g, MI355_ERR_INVALID_ARG, "group: null net");
  YxNetInfo info;
  yolox_net_info(net, &info);
  YdKind &k = g->yd.kind;
  for (auto it = k.infer_tickets.begin(); it != k.infer_tickets.end();) {
    if (!g->yd.owns(it->first)) { it = k.infer_tickets.erase(it); continue; }   // (a result nobody collected and the queue dropped)
    if (it->second == info.serial) return fail(g, MI355_ERR_INVALID_ARG, "group: a ticket that names this net is pending or uncollected");
    ++it;
  }
  if (!k.net_lanes) return MI355_OK;   // the queue has never been used
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  // every set that named the net has been collected, so it has finished; the wait is for what the stream may hold behind it
  if (hipStreamSynchronize(k.stream) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipStreamSynchronize(decoder queue)"); }
  (void)yolox_lanes_release(k.net_lanes, info.serial);
  return MI355_OK;
}

int mi355_group_yolox_infer_stats(mi355_group *g, uint64_t stats[6]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  const YdKind &k = g->yd.kind;
  stats[0] = k.n_infer;
  stats[1] = k.n_forwards;
  stats[2] = k.n_largest_forward;
  stats[3] = k.n_infer_launches;
  yolox_lanes_stats(k.net_lanes, &stats[4], &stats[5]);
  return MI355_OK;
}

int mi355_group_wait_yolodec(mi355_group *g, uint64_t ticket, mi355_yolo_det *dets, uint32_t *n_dets) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!n_dets) return fail(g, MI355_ERR_INVALID_ARG, "group: null result count");
  if (!dets) {
    // Only a tensor submitted with max_dets == 0 has no records to take. The refusal leaves the result collectable, so the
    // capacity is looked up wherever the tensor stands - pending, in a set in flight, or collected into `results` - and not by
    // taking the result out first. (A ticket that is not this queue's has no capacity here and is refused below.)
    const auto at = g->yd.find(ticket);
    const uint32_t cap = at.pending ? at.pending->max_dets : at.set ? at.set->data.slots[at.index].max_dets : at.result ? at.result->max_dets : 0;
    if (cap) return fail(g, MI355_ERR_INVALID_ARG, "group: null records for a tensor submitted with max_dets > 0");
  }
  YdOut res;
  const int rc = g->yd.wait(g, L.lk, ticket, &res);
  if (!g->yd.owns(ticket)) g->yd.kind.infer_tickets.erase(ticket);   // taken, or told its failure: no longer names a net
  if (rc) return rc;
  *n_dets = res.n_dets;
  if (dets && !res.dets.empty()) std::memcpy(dets, res.dets.data(), res.dets.size() * sizeof(mi355_yolo_det));
  return MI355_OK;
}

int mi355_group_yolodec_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::yd, stats); }

int mi355_group_yolox_head_stats(mi355_group *g, uint64_t stats[4]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  const YdKind &k = g->yd.kind;
  stats[0] = k.n_heads;
  stats[1] = k.n_head_sets;
  stats[2] = k.n_head_uploads;
  stats[3] = k.n_head_launches;
  return MI355_OK;
}

int mi355_group_set_handdec_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  return queue_set_rendezvous(g, &mi355_group::hn, expected_streams, linger_us);
}

// the two submits' common part: the lone entry points' checks for one tensor at a pitch equal to the tensor, in their order
static int submit_handdec(mi355_group *g, mi355_ctx *ctx, int decoder, const float *d_tensor, uint32_t rows, uint32_t kps_dim, const float *d_scores,
                          uint32_t num_scores, const mi355_hand_params *p, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !p || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context, settings or ticket");
  if (!d_scores) num_scores = 0;   // no scores: num_scores is ignored
  const char *why = nullptr;
  const size_t tensor_bytes = decoder == 0 ? (size_t)rows * 32 : (size_t)rows * 21 * kps_dim * 4;
  int rc = handdec_check_args(decoder, tensor_bytes, 1, rows, kps_dim, (size_t)num_scores * 4, num_scores, &why);
  if (!rc) rc = handdec_check_params(decoder, p->max_hands, p->frame_width, p->frame_height, &why);
  if (rc) return fail(g, rc, why);
  if (rows && (!d_tensor || (uintptr_t)d_tensor % 4 != 0 || (uintptr_t)d_scores % 4 != 0)) return fail(g, MI355_ERR_INVALID_ARG, "handdec: null or misaligned tensors");
  // a tensor without rows is not read: it does not make the set wait for its stream (the model's last kernel, an upload)
  return g->hn.submit(g, ctx, HnTensor{decoder, d_tensor, rows, kps_dim, d_scores, num_scores, *p}, rows != 0, ticket);
}

int mi355_group_submit_handdec_palm(mi355_group *g, mi355_ctx *ctx, const float *d_tensor, uint32_t num_rows, const mi355_hand_params *p, uint64_t *ticket) {
  return submit_handdec(g, ctx, 0, d_tensor, num_rows, 0, nullptr, 0, p, ticket);
}

int mi355_group_submit_handdec_landmarks(mi355_group *g, mi355_ctx *ctx, const float *d_landmarks, uint32_t num_hands, uint32_t kps_dim, const float *d_scores,
                                         uint32_t num_scores, const mi355_hand_params *p, uint64_t *ticket) {
  return submit_handdec(g, ctx, 1, d_landmarks, num_hands, kps_dim, d_scores, num_scores, p, ticket);
}

int mi355_group_wait_handdec(mi355_group *g, uint64_t ticket, mi355_hand_det *dets, mi355_hand_keypoints *kps, uint32_t *n_hands) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!dets || !n_hands) return fail(g, MI355_ERR_INVALID_ARG, "group: null result arrays");
  if (!kps) {
    // Only a palm ticket has no keypoint records to take. The refusal leaves the result collectable, so the decoder is looked up
    // wherever the tensor stands - pending, in a set in flight, or collected into `results` - and not by taking the result out
    // first. (A ticket that is not this queue's has no decoder here and is refused below.)
    const auto at = g->hn.find(ticket);
    const int decoder = at.pending ? at.pending->decoder : at.set ? at.set->data.slots[at.index].decoder : at.result ? at.result->decoder : 0;
    if (decoder == 1) return fail(g, MI355_ERR_INVALID_ARG, "group: null keypoint records for a landmark tensor");
  }
  HnOut res;
  if (int rc = g->hn.wait(g, L.lk, ticket, &res)) return rc;
  *n_hands = res.n_hands;
  if (!res.dets.empty()) std::memcpy(dets, res.dets.data(), res.dets.size() * sizeof(mi355_hand_det));
  if (!res.kps.empty()) std::memcpy(kps, res.kps.data(), res.kps.size() * sizeof(mi355_hand_keypoints));
  return MI355_OK;
}

int mi355_group_handdec_stats(mi355_group *g, uint64_t stats[4]) { return queue_stats(g, &mi355_group::hn, stats); }

int mi355_group_wait(mi355_group *g, uint64_t ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (ticket == 0 || ticket >= g->next_ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: unknown ticket");
  if (int rc = refuse_set_queue_ticket(g, ticket)) return rc;
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  bool is_pending = false;
  for (const Desc &d : g->pending) is_pending |= d.ticket == ticket;
  if (is_pending) {
    int rc = flush_locked(g, ticket);
    if (rc && g->failed.find(ticket) == g->failed.end()) return rc;  // (a failure of this frame's own batch is reported - once - below)
  }
  return wait_unlocking(g, lk, ticket);
}

int mi355_group_order_after(mi355_group *g, mi355_ctx *ctx, uint64_t ticket) {
  if (!g || !ctx) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (ticket == 0 || ticket >= g->next_ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: unknown ticket");
  if (int rc = refuse_set_queue_ticket(g, ticket)) return rc;
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  bool is_pending = false;
  for (const Desc &d : g->pending) is_pending |= d.ticket == ticket;
  if (is_pending) {
    int rc = flush_locked(g, ticket);
    if (rc) return rc;
  }
  auto bad = g->failed.find(ticket);
  if (bad != g->failed.end()) return fail(g, bad->second, "group: the launch that carried this frame failed");
  auto it = g->where.find(ticket);
  if (it == g->where.end()) return MI355_OK;  // retired: the frame is done, nothing to order
  for (Batch &b : g->batches)
    if (b.seq == it->second) {
      if (hipStreamWaitEvent(ctx->stream, b.done, 0) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipStreamWaitEvent(group batch)"); }
      break;
    }
  return MI355_OK;
}

int mi355_group_wait_all(mi355_group *g) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  int rc = flush_locked(g);
  if (rc) return rc;
  if ((rc = wait_all_unlocking(g, lk))) return rc;
  for_each_queue_but_compare(g, [&](auto &q) {   // each queue that has been set up, in turn; the first failure ends it
    if (rc || !q.kind.set_up()) return;
    if (!(rc = q.flush_locked(g))) rc = q.wait_all_unlocking(g, lk);
  });
  return rc;
}

int mi355_group_submit_round(mi355_group *g, mi355_ctx *const *ctxs, int n_streams, uint8_t *const *d_src, uint8_t *const *d_dst, int width, int height,
                             int stride, int format, const mi355_hsv_settings *settings) {
  if (!g || !ctxs || !d_src || !d_dst || n_streams < 0) return MI355_ERR_INVALID_ARG;
  for (int i = 0; i < n_streams; i++) {
    int rc = mi355_group_submit_chain(g, ctxs[i], d_src[i], d_dst[i], width, height, stride, format, settings, nullptr);
    if (rc) return rc;
  }
  return mi355_group_flush(g);
}

int mi355_group_submit_round_fused(mi355_group *g, mi355_ctx *const *ctxs, int n_streams, uint8_t *const *d_src, uint8_t *const *d_dst, int width,
                                   int height, int stride, int format, const mi355_hsv_settings *settings) {
  if (!g || !ctxs || !d_src || !d_dst || n_streams < 0) return MI355_ERR_INVALID_ARG;
  for (int i = 0; i < n_streams; i++) {
    int rc = mi355_group_submit_fused(g, ctxs[i], d_src[i], d_dst[i], width, height, stride, format, settings, nullptr);
    if (rc) return rc;
  }
  return mi355_group_flush(g);
}

int mi355_group_stats(mi355_group *g, uint64_t stats[3]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_frames;
  stats[1] = g->n_batched_launch_pairs;
  stats[2] = g->n_single;
  return MI355_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the process's group per device
// Elements of independent pipelines share nothing but the process: mi355_group_shared(device) is THE dispatcher of that device
// (created at first use, reference-counted: every call is paired with one mi355_group_release; the last release destroys it).
namespace {
std::mutex g_pg_mu;
struct ProcessGroup { int device; mi355_group *g; int refs; };
std::vector<ProcessGroup> g_pg;
}  // namespace

extern "C" {

mi355_group *mi355_group_shared(int device, int *status) {
  std::lock_guard<std::mutex> lk(g_pg_mu);
  for (ProcessGroup &p : g_pg)
    if (p.device == device) { p.refs++; if (status) *status = MI355_OK; return p.g; }
  mi355_group *g = mi355_group_create(device, 0, status);
  if (g) g_pg.push_back(ProcessGroup{device, g, 1});
  return g;
}

void mi355_group_release(mi355_group *g) {
  if (!g) return;
  bool last = false;
  {
    std::lock_guard<std::mutex> lk(g_pg_mu);
    for (size_t i = 0; i < g_pg.size(); i++)
      if (g_pg[i].g == g) {
        last = --g_pg[i].refs == 0;
        if (last) g_pg.erase(g_pg.begin() + (std::ptrdiff_t)i);
        break;
      }
  }
  if (last) mi355_group_destroy(g);
}

}  // extern "C"
