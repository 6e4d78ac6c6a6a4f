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
// Four more queues live beside the filter batches, each with its own HIP stream, pending list, rendezvous and stats, and none
// touching another: videocompare pairs (submit_compare), colordetect frames (submit_colordetect), hsvdetector frames
// (submit_hsvdetect: up to 32 frames of independent instances - own size, strides, formats, settings - as at most two launches
// over a job table, hsv_kernels.hip) and decoder tensors (submit_yolodec: up to 32 tensors of independent yolov8tensordec2 /
// yoloxtensordec instances - own shape, layout, settings - as at most three launches over job tables and one download,
// yolodec.hip). Tickets are one sequence; a wait entry refuses a ticket of another queue.
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

// ---- videocompare across independent element instances (mi355_group_submit_compare): one (reference frame, frame) pair per submit
struct CmpDesc {
  mi355_ctx *ctx;
  const uint8_t *ref, *frame;
  int width, height, stride, format, algo, translucent, fast;   // fast: MI355_FLAG_DSSIM_FAST of the submitting context
  uint64_t ticket;
  hipEvent_t ready;  // recorded on ctx->stream at submit (nullptr: the stream held nothing)
};
struct CmpResult { int status; double distance; uint64_t hashes[2]; };
struct CmpBatch {
  uint64_t seq;
  std::vector<uint64_t> tickets;
  int algo, width, height;
  int lane;        // which of the compare queue's streams carries it (batches of one lane finish in seq order)
  hipEvent_t done;
  int waiters;
  void *h_block;  // pinned: Dssim [n][15] doubles / Blockhash [2 n] u64 (reference hashes, then frame hashes)
  bool collected = false;  // its values are in cmp_results (the event and the block are recycled once nobody waits inside it)
};
constexpr int kCmpMaxBatch = 32;                      // pairs per launch set (a Dssim pair keeps 44 MB of maps until its batch is reduced)
constexpr int kCmpMaxLanes = 16;                      // HIP streams the pairs of one launch set are dealt out to
constexpr size_t kCmpBlockBytes = 64 * 15 * 8 + 1024; // one pinned result block

// ---- colordetect across independent element instances (mi355_group_submit_colordetect): one flat device plane per submit
struct CdDesc {
  CdFrame f;
  uint64_t ticket;
  hipEvent_t ready;  // recorded on the submitting context's stream (nullptr: the stream held nothing)
};
struct CdOut { int status, n_colors; uint8_t rgb[255 * 3]; };
struct CdSet {
  uint64_t seq;  // launch order on the queue's stream: set n is done => every set before it is
  std::vector<uint64_t> tickets;
  hipEvent_t done;
  int waiters;
  void *h_block;  // pinned: the set's results (colordetect_set_result)
  bool collected = false;
};
constexpr int kCdBlocksAtFirstUse = 4;  // pinned result blocks = launch sets in flight before one more has to be allocated


// ---- hsvdetector across independent element instances (mi355_group_submit_hsvdetect): one device frame per submit, written in
// place on the device - nothing comes back but the launch's status
struct HdDesc {
  HdFrame f;
  uint64_t ticket;
  hipEvent_t ready;  // recorded on the submitting context's stream (nullptr: the stream held nothing)
};
struct HdSet {
  uint64_t seq;  // launch order on the queue's stream: set n is done => every set before it is
  std::vector<uint64_t> tickets;
  hipEvent_t done;
  int waiters;
  bool collected = false;
};

// ---- yolov8tensordec2 / yoloxtensordec across independent element instances (mi355_group_submit_yolodec): one device tensor per
// submit; its kept count and records come back through the set's pinned block
struct YdDesc {
  YdTensor t;
  uint64_t ticket;
  hipEvent_t ready;  // recorded on the submitting context's stream (nullptr: the stream held nothing, or no candidate to read)
};
struct YdOut { int status; uint32_t n_dets, max_dets; std::vector<mi355_yolo_det> dets; };   // dets: the first min(n_dets, max_dets)
struct YdBlock { void *h; size_t bytes; };   // a pinned result block
struct YdSlot { uint64_t ticket; uint32_t num_candidates, max_dets; uint64_t det_offset; };
struct YdSet {
  uint64_t seq;  // launch order on the queue's stream: set n is done => every set before it is
  std::vector<YdSlot> slots;   // its tensors, by job
  hipEvent_t done;
  int waiters;
  YdBlock block;     // the set's own results until it is collected (h == nullptr: no tensor had a candidate)
  bool collected = false;
};

}  // namespace

struct mi355_group {
  int device = 0;
  int max_batch = 8;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::vector<Desc> pending;
  std::deque<Batch> batches;       // launched, oldest first
  std::vector<hipEvent_t> events;  // free list
  std::unordered_map<uint64_t, uint64_t> where;  // ticket -> seq of its batch, for launched batches not yet retired
  std::unordered_map<uint64_t, int> failed;      // ticket -> status of the launch that did not happen (reported by wait / order_after)
  uint64_t next_ticket = 1, next_seq = 1;
  uint64_t n_frames = 0, n_batched_launch_pairs = 0, n_single = 0;
  std::string last_error;
  // table references of retired batches: dropping the last reference to a table frees 64 MiB behind a device-wide wait, which
  // does not belong under `mu` - the entry points empty this list into a local one that dies after they have unlocked (Locked)
  std::vector<std::shared_ptr<void>> dead_refs;
  // ---- compare queue (videocompare's Dssim / Blockhash): its own context + stream, independent of the filter batches above
  // The pairs of a launch set are dealt out to `n_lanes` contexts (streams): the Dssim kernels are VALU-bound at ~80 % busy when
  // one runs alone, and a second stream's launches fill its tails and launch boundaries (32 4K pairs: 1.48 k comparisons/s on one
  // stream, 1.84 k over eight) - what the dispatcher removes is the per-comparison host round trip, not the overlap.
  mi355_ctx *alane[kCmpMaxLanes] = {nullptr};
  int n_lanes = 8;
  mi355_ctx *actx = nullptr;                 // = alane[0], created at the first compare submit
  std::vector<CmpDesc> cmp_pending;
  std::deque<CmpBatch> cmp_batches;          // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> cmp_where;      // ticket -> seq
  std::unordered_map<uint64_t, CmpResult> cmp_results;   // finished, not yet collected by mi355_group_wait_compare
  std::vector<void *> cmp_blocks;            // free pinned result blocks
  uint32_t *d_hash_sums[kCmpMaxLanes] = {nullptr};   // Blockhash scratch per lane: [2 kCmpMaxBatch][64] u32 + [2 kCmpMaxBatch] u64
  uint64_t next_cmp_seq = 1;
  uint64_t n_cmp_pairs = 0, n_cmp_batches = 0, n_cmp_largest = 0;
  int expected_streams = 0;                  // rendezvous: a waiter lingers until this many pairs are pending ...
  unsigned linger_us = 0;                    // ... or this long (mi355_group_set_rendezvous)
  std::condition_variable cv;                // "a compare batch has been launched"
  // ---- colordetect queue: its own stream and scratch (created at the first submit), independent of the two queues above
  hipStream_t cd_stream = nullptr;
  CdSetScratch *cd_scratch = nullptr;
  int cd_n_cu = 256;
  std::vector<CdDesc> cd_pending;
  std::deque<CdSet> cd_sets;                 // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> cd_where;   // ticket -> seq
  std::unordered_map<uint64_t, CdOut> cd_results;    // finished (or failed), not yet collected by mi355_group_wait_colordetect
  std::vector<void *> cd_blocks;             // free pinned result blocks
  uint64_t next_cd_seq = 1;
  uint64_t n_cd_frames = 0, n_cd_sets = 0, n_cd_largest = 0, n_cd_launches = 0;
  int cd_expected = 0;                       // rendezvous over pending colordetect frames (mi355_group_set_colordetect_rendezvous)
  unsigned cd_linger_us = 0;
  std::condition_variable cd_cv;             // "a colordetect set has been launched"
  // ---- hsvdetector queue: its own stream (created at the first submit), independent of the three queues above
  hipStream_t hd_stream = nullptr;
  int hd_n_cu = 256;
  std::vector<HdDesc> hd_pending;
  std::deque<HdSet> hd_sets;                 // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> hd_where;   // ticket -> seq
  std::unordered_map<uint64_t, int> hd_results;      // status of frames finished (or failed), not yet collected by mi355_group_wait_hsvdetect
  uint64_t next_hd_seq = 1;
  uint64_t n_hd_frames = 0, n_hd_sets = 0, n_hd_largest = 0, n_hd_launches = 0;
  int hd_expected = 0;                       // rendezvous over pending detector frames (mi355_group_set_hsvdetect_rendezvous)
  unsigned hd_linger_us = 0;
  std::condition_variable hd_cv;             // "a detector set has been launched"
  // ---- decoder queue: its own stream and scratch (created at the first submit), independent of the four queues above
  hipStream_t yd_stream = nullptr;
  YdSetScratch *yd_scratch = nullptr;
  std::vector<YdDesc> yd_pending;
  std::deque<YdSet> yd_sets;                 // launched, oldest first
  std::unordered_map<uint64_t, uint64_t> yd_where;   // ticket -> seq
  std::unordered_map<uint64_t, YdOut> yd_results;    // finished (or failed), not yet collected by mi355_group_wait_yolodec
  std::vector<YdBlock> yd_blocks;            // free pinned result blocks
  uint64_t next_yd_seq = 1;
  uint64_t n_yd_tensors = 0, n_yd_sets = 0, n_yd_largest = 0, n_yd_launches = 0;
  int yd_expected = 0;                       // rendezvous over pending tensors (mi355_group_set_yolodec_rendezvous)
  unsigned yd_linger_us = 0;
  std::condition_variable yd_cv;             // "a decoder set has been launched"
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

hipEvent_t take_event(mi355_group *g) {
  if (!g->events.empty()) { hipEvent_t e = g->events.back(); g->events.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return e;
}

int fail(mi355_group *g, int status, const std::string &msg) {
  g->last_error = msg;
  return status;
}

bool same_class(const Desc &a, const Desc &b) {
  return a.batchable && b.batchable && a.fused == b.fused && a.width == b.width && a.height == b.height && a.stride == b.stride && a.format == b.format && a.table == b.table &&
         std::memcmp(&a.hs, &b.hs, sizeof(a.hs)) == 0 && a.ctx->force_generic == b.ctx->force_generic;
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
  Batch *mine = nullptr;
  for (Batch &b : g->batches)
    if (b.seq == seq) { mine = &b; break; }
  if (!mine) return MI355_OK;
  const hipEvent_t ev = mine->done;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (Batch &b : g->batches)
    if (b.seq == seq) { b.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group batch)"); }
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

// ------------------------------------------------------------------ compare queue

void *cmp_take_block(mi355_group *g) {
  if (!g->cmp_blocks.empty()) { void *b = g->cmp_blocks.back(); g->cmp_blocks.pop_back(); return b; }
  void *b = nullptr;
  if (hipHostMalloc(&b, kCmpBlockBytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return b;
}

bool cmp_same_class(const CmpDesc &a, const CmpDesc &b) {
  return a.algo == b.algo && a.width == b.width && a.height == b.height && a.stride == b.stride && a.format == b.format && a.translucent == b.translucent && a.fast == b.fast;
}

// a finished batch: values from its pinned block into cmp_results (once). g->mu held.
void cmp_collect(mi355_group *g, CmpBatch &b) {
  if (b.collected) return;
  b.collected = true;
  const int n = (int)b.tickets.size();
  if (b.algo == MI355_HASH_DSSIM) {
    std::vector<double> v((size_t)n);
    dssim_scores_from_slots(b.width, b.height, (const double *)b.h_block, n, v.data());
    for (int i = 0; i < n; i++) g->cmp_results[b.tickets[i]] = CmpResult{MI355_OK, v[i], {0, 0}};
  } else {
    const uint64_t *h = (const uint64_t *)b.h_block;
    for (int i = 0; i < n; i++)
      g->cmp_results[b.tickets[i]] = CmpResult{MI355_OK, mi355_videocompare_distance(MI355_HASH_BLOCKHASH, h[i], h[n + i]), {h[i], h[n + i]}};
  }
  for (uint64_t t : b.tickets) g->cmp_where.erase(t);
}

// collected batches nobody waits inside leave from the front: event and pinned block back to their free lists. g->mu held.
void cmp_retire(mi355_group *g) {
  for (auto it = g->cmp_batches.begin(); it != g->cmp_batches.end();) {
    if (it->collected && it->waiters == 0) {
      g->cmp_blocks.push_back(it->h_block);
      g->events.push_back(it->done);
      it = g->cmp_batches.erase(it);
    } else {
      ++it;
    }
  }
}

// launches the pending pairs, class by class (all of them, or up to the batch that carries `until`): the pairs of a class are
// dealt out to the lanes in contiguous shares (pairs that share a reference frame stay together). g->mu held.
int cmp_flush_locked(mi355_group *g, uint64_t until = 0) {
  bool reached = false;
  int first_rc = MI355_OK;
  while (!g->cmp_pending.empty() && !reached) {
    std::vector<CmpDesc> all, keep;
    const CmpDesc first = g->cmp_pending.front();
    for (const CmpDesc &d : g->cmp_pending) {
      if ((int)all.size() < kCmpMaxBatch && cmp_same_class(first, d)) all.push_back(d);
      else keep.push_back(d);
    }
    g->cmp_pending.swap(keep);
    // pairs that share a reference frame next to each other (videocompare with several pads: the reference is hashed once)
    std::stable_sort(all.begin(), all.end(), [](const CmpDesc &a, const CmpDesc &b) { return (uintptr_t)a.ref < (uintptr_t)b.ref; });
    const int total = (int)all.size();
    const int lanes = total < g->n_lanes ? total : g->n_lanes;
    PixFmt fmt;
    (void)pixfmt_of(first.format, &fmt);
    int begin = 0;
    for (int lane = 0; lane < lanes; lane++) {
      int end = (int)((long long)total * (lane + 1) / lanes);
      // a reference frame is not split over two lanes
      while (end < total && end > begin && all[end].ref == all[end - 1].ref) end++;
      if (end <= begin) continue;
      std::vector<CmpDesc> take(all.begin() + begin, all.begin() + end);
      begin = end;
      const int n = (int)take.size();
      mi355_ctx *a = g->alane[lane];
      int rc = MI355_OK;
      hipEvent_t done = take_event(g);
      void *block = cmp_take_block(g);
      if (!done || !block) rc = MI355_ERR_HIP;
      for (const CmpDesc &d : take)
        if (!rc && d.ready && hipStreamWaitEvent(a->stream, d.ready, 0) != hipSuccess) rc = MI355_ERR_HIP;
      std::vector<const uint8_t *> refs((size_t)n), frames((size_t)n);
      for (int i = 0; i < n; i++) { refs[i] = take[i].ref; frames[i] = take[i].frame; }
      if (!rc && first.algo == MI355_HASH_DSSIM) {
        a->dssim_translucent = first.translucent;
        a->dssim_fast = first.fast;   // a batch holds pairs of one form only (cmp_same_class)
        rc = dssim_compare_pairs_enqueue(a, refs.data(), frames.data(), n, first.stride, first.width, first.height, fmt.pixel_stride, (double *)block);
      } else if (!rc) {
        std::vector<const uint8_t *> both(refs);
        both.insert(both.end(), frames.begin(), frames.end());
        unsigned long long *d_hashes = (unsigned long long *)(g->d_hash_sums[lane] + (size_t)2 * kCmpMaxBatch * 64);
        rc = blockhash_enqueue(a, both.data(), 2 * n, first.stride, first.width, first.height, fmt.pixel_stride, g->d_hash_sums[lane], d_hashes);
        if (!rc && hipMemcpyAsync(block, d_hashes, (size_t)2 * n * 8, hipMemcpyDeviceToHost, a->stream) != hipSuccess) rc = MI355_ERR_HIP;
      }
      if (!rc && hipEventRecord(done, a->stream) != hipSuccess) rc = MI355_ERR_HIP;
      if (rc) {
        (void)hipGetLastError();
        if (done) g->events.push_back(done);
        if (block) g->cmp_blocks.push_back(block);
        g->last_error = a->last_error.empty() ? "group: compare launch failed" : a->last_error;
        if (g->cmp_results.size() > 65536) g->cmp_results.clear();   // (results nobody ever collected)
        for (const CmpDesc &d : take) g->cmp_results[d.ticket] = CmpResult{rc, 0.0, {0, 0}};   // told to the pair's own wait, once
        if (!first_rc) first_rc = rc;
        continue;
      }
      CmpBatch b{g->next_cmp_seq++, {}, first.algo, first.width, first.height, lane, done, 0, block};
      for (const CmpDesc &d : take) { b.tickets.push_back(d.ticket); g->cmp_where[d.ticket] = b.seq; reached |= until != 0 && d.ticket == until; }
      g->cmp_batches.push_back(std::move(b));
    }
    for (const CmpDesc &d : all)
      if (d.ready) g->events.push_back(d.ready);
    g->n_cmp_pairs += (uint64_t)total;
    g->n_cmp_batches++;
    if ((uint64_t)total > g->n_cmp_largest) g->n_cmp_largest = (uint64_t)total;
  }
  g->cv.notify_all();
  return first_rc;
}

// finished batches are collected without a waiter (their results stay in cmp_results until asked for)
void cmp_retire_done(mi355_group *g) {
  for (CmpBatch &b : g->cmp_batches) {
    if (b.collected) continue;
    if (hipEventQuery(b.done) != hipSuccess) { (void)hipGetLastError(); continue; }   // (the lanes finish independently)
    cmp_collect(g, b);
  }
  cmp_retire(g);
}

// host wait for the batch of `ticket`; `lk` owns g->mu on entry and on return, not while waiting
int cmp_wait_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
  auto it = g->cmp_where.find(ticket);
  if (it == g->cmp_where.end()) return MI355_OK;  // collected already (or failed: cmp_results has it)
  const uint64_t seq = it->second;
  CmpBatch *mine = nullptr;
  for (CmpBatch &b : g->cmp_batches)
    if (b.seq == seq) { mine = &b; break; }
  if (!mine) return MI355_OK;
  const hipEvent_t ev = mine->done;
  const int lane = mine->lane;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (CmpBatch &b : g->cmp_batches)
    if (b.seq == seq) { b.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group compare batch)"); }
  // a lane's stream is in order: everything of that lane up to this batch is done
  for (CmpBatch &b : g->cmp_batches)
    if (b.lane == lane && b.seq <= seq) cmp_collect(g, b);
  cmp_retire(g);
  return MI355_OK;
}

// ------------------------------------------------------------------ colordetect queue

// is `ticket` a colordetect frame that has not been collected?
bool cd_owns(mi355_group *g, uint64_t ticket) {
  if (g->cd_where.count(ticket) || g->cd_results.count(ticket)) return true;
  for (const CdDesc &d : g->cd_pending)
    if (d.ticket == ticket) return true;
  return false;
}

// stream, device scratch and the first pinned blocks: at the first submit, never inside a launch set. g->mu held.
int cd_ensure(mi355_group *g) {
  if (g->cd_scratch) return MI355_OK;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess) (void)hipGetLastError();
  g->cd_n_cu = n_cu > 0 ? n_cu : 256;
  if (!g->cd_stream && hipStreamCreateWithFlags(&g->cd_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    g->cd_stream = nullptr;
    return fail(g, MI355_ERR_HIP, "group: no stream for the colordetect queue");
  }
  while ((int)g->cd_blocks.size() < kCdBlocksAtFirstUse) {
    void *b = nullptr;
    if (hipHostMalloc(&b, colordetect_set_block_bytes(), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(g, MI355_ERR_OUT_OF_MEMORY, "group: no pinned result blocks for the colordetect queue");
    }
    g->cd_blocks.push_back(b);
  }
  int st = MI355_OK;
  std::string err;
  g->cd_scratch = colordetect_set_scratch_new(g->cd_stream, &st, &err);
  return g->cd_scratch ? MI355_OK : fail(g, st, "group: " + err);
}

// a finished set: its palettes from the pinned block into cd_results (once). g->mu held.
void cd_collect(mi355_group *g, CdSet &s) {
  if (s.collected) return;
  s.collected = true;
  if (g->cd_results.size() > 65536) g->cd_results.clear();   // (results nobody ever collected)
  for (size_t i = 0; i < s.tickets.size(); i++) {
    CdOut &o = g->cd_results[s.tickets[i]];
    o.status = MI355_OK;
    colordetect_set_result(s.h_block, (int)i, o.rgb, &o.n_colors);
    g->cd_where.erase(s.tickets[i]);
  }
}

// collected sets nobody waits inside leave: event and pinned block back to their free lists. g->mu held.
void cd_retire(mi355_group *g) {
  for (auto it = g->cd_sets.begin(); it != g->cd_sets.end();) {
    if (it->collected && it->waiters == 0) {
      g->cd_blocks.push_back(it->h_block);
      g->events.push_back(it->done);
      it = g->cd_sets.erase(it);
    } else {
      ++it;
    }
  }
}

// finished sets are collected without a waiter (the queue's stream is in order: the first unfinished set ends the search)
void cd_retire_done(mi355_group *g) {
  for (CdSet &s : g->cd_sets) {
    if (s.collected) continue;
    if (hipEventQuery(s.done) != hipSuccess) { (void)hipGetLastError(); break; }
    cd_collect(g, s);
  }
  cd_retire(g);
}

// launches the pending frames in submission order, kCdSetMax to a set (all of them, or up to the set that carries `until`):
// consecutive sets on the queue's stream share the scratch, each has its own pinned block. g->mu held.
int cd_flush_locked(mi355_group *g, uint64_t until = 0) {
  bool reached = false;
  int first_rc = MI355_OK;
  while (!g->cd_pending.empty() && !reached) {
    const size_t n = std::min(g->cd_pending.size(), (size_t)kCdSetMax);
    std::vector<CdDesc> take(g->cd_pending.begin(), g->cd_pending.begin() + (std::ptrdiff_t)n);
    g->cd_pending.erase(g->cd_pending.begin(), g->cd_pending.begin() + (std::ptrdiff_t)n);
    int rc = MI355_OK, launches = 0;
    std::string err;
    hipEvent_t done = take_event(g);
    if (g->cd_blocks.empty()) cd_retire_done(g);
    void *block = nullptr;
    if (!g->cd_blocks.empty()) { block = g->cd_blocks.back(); g->cd_blocks.pop_back(); }
    // (more sets in flight than ever before: one more block, kept from then on)
    else if (hipHostMalloc(&block, colordetect_set_block_bytes(), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); block = nullptr; }
    if (!done || !block) { rc = MI355_ERR_HIP; err = "group: no event or pinned block for a colordetect set"; }
    CdFrame frames[kCdSetMax];
    for (size_t i = 0; i < n; i++) {
      frames[i] = take[i].f;
      if (!rc && take[i].ready && hipStreamWaitEvent(g->cd_stream, take[i].ready, 0) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipStreamWaitEvent(colordetect frame)"; }
    }
    if (!rc) rc = colordetect_launch_set(g->cd_scratch, g->cd_stream, g->cd_n_cu, frames, (int)n, block, &launches, &err);
    if (!rc && hipEventRecord(done, g->cd_stream) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipEventRecord(colordetect set)"; }
    for (const CdDesc &d : take)
      if (d.ready) g->events.push_back(d.ready);
    if (rc) {
      (void)hipGetLastError();
      if (done) g->events.push_back(done);
      if (block) g->cd_blocks.push_back(block);
      g->last_error = "group: colordetect launch failed: " + err;
      if (g->cd_results.size() > 65536) g->cd_results.clear();
      for (const CdDesc &d : take) {   // told to the frame's own wait, once
        CdOut &o = g->cd_results[d.ticket];
        o.status = rc;
        o.n_colors = 0;
      }
      if (!first_rc) first_rc = rc;
      continue;
    }
    CdSet s{g->next_cd_seq++, {}, done, 0, block};
    for (const CdDesc &d : take) { s.tickets.push_back(d.ticket); g->cd_where[d.ticket] = s.seq; reached |= until != 0 && d.ticket == until; }
    g->cd_sets.push_back(std::move(s));
    g->n_cd_frames += n;
    g->n_cd_sets++;
    if (n > g->n_cd_largest) g->n_cd_largest = n;
    g->n_cd_launches += (uint64_t)launches;
  }
  g->cd_cv.notify_all();
  return first_rc;
}

// host wait for the set of `ticket`; `lk` owns g->mu on entry and on return, not while waiting
int cd_wait_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
  auto it = g->cd_where.find(ticket);
  if (it == g->cd_where.end()) return MI355_OK;  // collected already (or failed: cd_results has it)
  const uint64_t seq = it->second;
  CdSet *mine = nullptr;
  for (CdSet &s : g->cd_sets)
    if (s.seq == seq) { mine = &s; break; }
  if (!mine) return MI355_OK;
  const hipEvent_t ev = mine->done;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (CdSet &s : g->cd_sets)
    if (s.seq == seq) { s.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group colordetect set)"); }
  for (CdSet &s : g->cd_sets)
    if (s.seq <= seq) cd_collect(g, s);
  cd_retire(g);
  return MI355_OK;
}

// waits for every set launched so far (their results stay collectable)
int cd_wait_all_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk) {
  uint64_t last = 0;
  for (const CdSet &s : g->cd_sets)
    if (!s.collected) last = s.tickets.front();
  return last ? cd_wait_unlocking(g, lk, last) : MI355_OK;
}

// ------------------------------------------------------------------ hsvdetector queue

// is `ticket` a detector frame that has not been collected?
bool hd_owns(mi355_group *g, uint64_t ticket) {
  if (g->hd_where.count(ticket) || g->hd_results.count(ticket)) return true;
  for (const HdDesc &d : g->hd_pending)
    if (d.ticket == ticket) return true;
  return false;
}

// the queue's stream: at the first submit, never inside a launch set. g->mu held.
int hd_ensure(mi355_group *g) {
  if (g->hd_stream) return MI355_OK;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess) (void)hipGetLastError();
  g->hd_n_cu = n_cu > 0 ? n_cu : 256;
  if (hipStreamCreateWithFlags(&g->hd_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    g->hd_stream = nullptr;
    return fail(g, MI355_ERR_HIP, "group: no stream for the hsvdetector queue");
  }
  return MI355_OK;
}

// a finished set: its frames become collectable (once). g->mu held.
void hd_collect(mi355_group *g, HdSet &s) {
  if (s.collected) return;
  s.collected = true;
  if (g->hd_results.size() > 65536) g->hd_results.clear();   // (results nobody ever collected)
  for (uint64_t t : s.tickets) {
    g->hd_results[t] = MI355_OK;
    g->hd_where.erase(t);
  }
}

// collected sets nobody waits inside leave: the event goes back to the free list. g->mu held.
void hd_retire(mi355_group *g) {
  for (auto it = g->hd_sets.begin(); it != g->hd_sets.end();) {
    if (it->collected && it->waiters == 0) {
      g->events.push_back(it->done);
      it = g->hd_sets.erase(it);
    } else {
      ++it;
    }
  }
}

// finished sets are collected without a waiter (the queue's stream is in order: the first unfinished set ends the search)
void hd_retire_done(mi355_group *g) {
  for (HdSet &s : g->hd_sets) {
    if (s.collected) continue;
    if (hipEventQuery(s.done) != hipSuccess) { (void)hipGetLastError(); break; }
    hd_collect(g, s);
  }
  hd_retire(g);
}

// launches the pending frames in submission order, kHdSetMax to a set (all of them, or up to the set that carries `until`), as
// consecutive sets on the queue's stream. g->mu held.
int hd_flush_locked(mi355_group *g, uint64_t until = 0) {
  bool reached = false;
  int first_rc = MI355_OK;
  while (!g->hd_pending.empty() && !reached) {
    const size_t n = std::min(g->hd_pending.size(), (size_t)kHdSetMax);
    std::vector<HdDesc> take(g->hd_pending.begin(), g->hd_pending.begin() + (std::ptrdiff_t)n);
    g->hd_pending.erase(g->hd_pending.begin(), g->hd_pending.begin() + (std::ptrdiff_t)n);
    int rc = MI355_OK, launches = 0;
    std::string err;
    hipEvent_t done = take_event(g);
    if (!done) { rc = MI355_ERR_HIP; err = "group: no event for a hsvdetector set"; }
    HdFrame frames[kHdSetMax];
    for (size_t i = 0; i < n; i++) {
      frames[i] = take[i].f;
      if (!rc && take[i].ready && hipStreamWaitEvent(g->hd_stream, take[i].ready, 0) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipStreamWaitEvent(hsvdetector frame)"; }
    }
    if (!rc) rc = hsvdetect_launch_set(g->hd_stream, g->hd_n_cu, frames, (int)n, &launches, &err);
    if (!rc && hipEventRecord(done, g->hd_stream) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipEventRecord(hsvdetector set)"; }
    for (const HdDesc &d : take)
      if (d.ready) g->events.push_back(d.ready);
    if (rc) {
      (void)hipGetLastError();
      if (done) g->events.push_back(done);
      g->last_error = "group: hsvdetector launch failed: " + err;
      if (g->hd_results.size() > 65536) g->hd_results.clear();
      for (const HdDesc &d : take) g->hd_results[d.ticket] = rc;   // told to the frame's own wait, once
      if (!first_rc) first_rc = rc;
      continue;
    }
    HdSet s{g->next_hd_seq++, {}, done, 0};
    for (const HdDesc &d : take) {
      s.tickets.push_back(d.ticket);
      g->hd_where[d.ticket] = s.seq;
      reached |= until != 0 && d.ticket == until;
      // what the element behind finds on-die, as the lone entry records it
      if (d.f.width > 0 && d.f.height > 0) note_written(g->device, d.f.dst, (size_t)d.f.dst_stride * (size_t)d.f.height);
    }
    g->hd_sets.push_back(std::move(s));
    g->n_hd_frames += n;
    g->n_hd_sets++;
    if (n > g->n_hd_largest) g->n_hd_largest = n;
    g->n_hd_launches += (uint64_t)launches;
  }
  g->hd_cv.notify_all();
  return first_rc;
}

// host wait for the set of `ticket`; `lk` owns g->mu on entry and on return, not while waiting
int hd_wait_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
  auto it = g->hd_where.find(ticket);
  if (it == g->hd_where.end()) return MI355_OK;  // collected already (or failed: hd_results has it)
  const uint64_t seq = it->second;
  HdSet *mine = nullptr;
  for (HdSet &s : g->hd_sets)
    if (s.seq == seq) { mine = &s; break; }
  if (!mine) return MI355_OK;
  const hipEvent_t ev = mine->done;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (HdSet &s : g->hd_sets)
    if (s.seq == seq) { s.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group hsvdetector set)"); }
  for (HdSet &s : g->hd_sets)
    if (s.seq <= seq) hd_collect(g, s);
  hd_retire(g);
  return MI355_OK;
}

// waits for every set launched so far (their frames stay collectable)
int hd_wait_all_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk) {
  uint64_t last = 0;
  for (const HdSet &s : g->hd_sets)
    if (!s.collected) last = s.tickets.front();
  return last ? hd_wait_unlocking(g, lk, last) : MI355_OK;
}

// ------------------------------------------------------------------ decoder queue

// is `ticket` a decoder tensor that has not been collected?
bool yd_owns(mi355_group *g, uint64_t ticket) {
  if (g->yd_where.count(ticket) || g->yd_results.count(ticket)) return true;
  for (const YdDesc &d : g->yd_pending)
    if (d.ticket == ticket) return true;
  return false;
}

// the queue's stream and scratch: at the first submit, never inside a launch set. g->mu held.
int yd_ensure(mi355_group *g) {
  if (g->yd_scratch) return MI355_OK;
  if (!g->yd_stream && hipStreamCreateWithFlags(&g->yd_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    g->yd_stream = nullptr;
    return fail(g, MI355_ERR_HIP, "group: no stream for the decoder queue");
  }
  int st = MI355_OK;
  std::string err;
  g->yd_scratch = yolodec_set_scratch_new(&st, &err);
  return g->yd_scratch ? MI355_OK : fail(g, st, "group: " + err);
}

// a pinned block of at least `bytes`: a free one that is large enough, else a new one (a free one that is too small makes room)
YdBlock yd_take_block(mi355_group *g, size_t bytes) {
  for (size_t i = 0; i < g->yd_blocks.size(); i++)
    if (g->yd_blocks[i].bytes >= bytes) {
      const YdBlock b = g->yd_blocks[i];
      g->yd_blocks.erase(g->yd_blocks.begin() + (std::ptrdiff_t)i);
      return b;
    }
  if (!g->yd_blocks.empty()) {
    (void)hipHostFree(g->yd_blocks.back().h);
    g->yd_blocks.pop_back();
  }
  YdBlock b{nullptr, 0};
  const size_t want = (bytes + 4095) / 4096 * 4096;
  if (hipHostMalloc(&b.h, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); b.h = nullptr; return b; }
  b.bytes = want;
  return b;
}

// a finished set: counts and records move from its pinned block into yd_results (once), the block is free again. g->mu held.
void yd_collect(mi355_group *g, YdSet &s) {
  if (s.collected) return;
  s.collected = true;
  if (g->yd_results.size() > 65536) g->yd_results.clear();   // (results nobody ever collected)
  const uint32_t *h_n = static_cast<const uint32_t *>(s.block.h);
  const mi355_yolo_det *h_dets = s.block.h ? reinterpret_cast<const mi355_yolo_det *>(static_cast<const uint8_t *>(s.block.h) + kYdCountsBytes) : nullptr;
  for (size_t i = 0; i < s.slots.size(); i++) {
    const YdSlot &sl = s.slots[i];
    YdOut &o = g->yd_results[sl.ticket];
    o.status = MI355_OK;
    o.max_dets = sl.max_dets;
    o.n_dets = sl.num_candidates && h_n ? h_n[i] : 0;   // a tensor without candidates had no job
    const uint32_t cap = sl.max_dets < sl.num_candidates ? sl.max_dets : sl.num_candidates;
    const uint32_t w = o.n_dets < cap ? o.n_dets : cap;
    if (w) o.dets.assign(h_dets + sl.det_offset, h_dets + sl.det_offset + w);
    g->yd_where.erase(sl.ticket);
  }
  if (s.block.h) g->yd_blocks.push_back(s.block);
  s.block = YdBlock{nullptr, 0};
}

// collected sets nobody waits inside leave: the event goes back to the free list. g->mu held.
void yd_retire(mi355_group *g) {
  for (auto it = g->yd_sets.begin(); it != g->yd_sets.end();) {
    if (it->collected && it->waiters == 0) {
      g->events.push_back(it->done);
      it = g->yd_sets.erase(it);
    } else {
      ++it;
    }
  }
}

// finished sets are collected without a waiter (the queue's stream is in order: the first unfinished set ends the search)
void yd_retire_done(mi355_group *g) {
  for (YdSet &s : g->yd_sets) {
    if (s.collected) continue;
    if (hipEventQuery(s.done) != hipSuccess) { (void)hipGetLastError(); break; }
    yd_collect(g, s);
  }
  yd_retire(g);
}

// launches the pending tensors in submission order, kYdSetMax to a set (all of them, or up to the set that carries `until`):
// consecutive sets on the queue's stream share the device scratch, each has its own pinned block. g->mu held.
int yd_flush_locked(mi355_group *g, uint64_t until = 0) {
  bool reached = false;
  int first_rc = MI355_OK;
  while (!g->yd_pending.empty() && !reached) {
    const size_t n = std::min(g->yd_pending.size(), (size_t)kYdSetMax);
    std::vector<YdDesc> take(g->yd_pending.begin(), g->yd_pending.begin() + (std::ptrdiff_t)n);
    g->yd_pending.erase(g->yd_pending.begin(), g->yd_pending.begin() + (std::ptrdiff_t)n);
    int rc = MI355_OK, launches = 0;
    std::string err;
    // the set's layout: the plan the launch itself uses
    YdTensor tensors[kYdSetMax];
    int layout[kYdSetMax];
    uint32_t F[kYdSetMax], N[kYdSetMax], cap[kYdSetMax], first[kYdSetMax], blocks[kYdSetMax];
    uint64_t key_off[kYdSetMax], box_off[kYdSetMax], det_off[kYdSetMax], totals[6] = {0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
      tensors[i] = take[i].t;
      layout[i] = take[i].t.layout; F[i] = take[i].t.num_fields; N[i] = take[i].t.num_candidates; cap[i] = take[i].t.max_dets;
    }
    rc = yolodec_set_plan((int)n, layout, F, N, cap, first, blocks, key_off, box_off, det_off, totals);
    if (rc) err = "group: bad decoder set";
    hipEvent_t done = take_event(g);
    YdBlock block{nullptr, 0};
    if (!rc && totals[2]) {   // a set without a candidate has nothing to copy
      if (g->yd_blocks.empty()) yd_retire_done(g);
      block = yd_take_block(g, yolodec_set_result_bytes(totals[5]));
    }
    if (!rc && (!done || (totals[2] && !block.h))) { rc = MI355_ERR_HIP; err = "group: no event or pinned block for a decoder set"; }
    for (size_t i = 0; i < n; i++)
      if (!rc && take[i].ready && hipStreamWaitEvent(g->yd_stream, take[i].ready, 0) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipStreamWaitEvent(decoder tensor)"; }
    if (!rc) rc = yolodec_launch_set(g->yd_scratch, g->yd_stream, tensors, (int)n, block.h, block.bytes, &launches, &err);
    if (!rc && hipEventRecord(done, g->yd_stream) != hipSuccess) { rc = MI355_ERR_HIP; err = "hipEventRecord(decoder set)"; }
    for (const YdDesc &d : take)
      if (d.ready) g->events.push_back(d.ready);
    if (rc) {
      (void)hipGetLastError();
      if (done) g->events.push_back(done);
      if (block.h) {
        // what did go out may still write the block: it is free again only behind the queue's stream
        (void)hipStreamSynchronize(g->yd_stream);
        (void)hipGetLastError();
        g->yd_blocks.push_back(block);
      }
      g->last_error = "group: decoder launch failed: " + err;
      if (g->yd_results.size() > 65536) g->yd_results.clear();
      for (const YdDesc &d : take) {   // told to the tensor's own wait, once
        YdOut &o = g->yd_results[d.ticket];
        o.status = rc;
        o.n_dets = 0;
        o.max_dets = d.t.max_dets;
      }
      if (!first_rc) first_rc = rc;
      continue;
    }
    YdSet s{g->next_yd_seq++, {}, done, 0, block};
    for (size_t i = 0; i < n; i++) {
      const YdDesc &d = take[i];
      s.slots.push_back(YdSlot{d.ticket, d.t.num_candidates, d.t.max_dets, det_off[i]});
      g->yd_where[d.ticket] = s.seq;
      reached |= until != 0 && d.ticket == until;
    }
    g->yd_sets.push_back(std::move(s));
    g->n_yd_tensors += n;
    g->n_yd_sets++;
    if (n > g->n_yd_largest) g->n_yd_largest = n;
    g->n_yd_launches += (uint64_t)launches;
  }
  g->yd_cv.notify_all();
  return first_rc;
}

// host wait for the set of `ticket`; `lk` owns g->mu on entry and on return, not while waiting
int yd_wait_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk, uint64_t ticket) {
  auto it = g->yd_where.find(ticket);
  if (it == g->yd_where.end()) return MI355_OK;  // collected already (or failed: yd_results has it)
  const uint64_t seq = it->second;
  YdSet *mine = nullptr;
  for (YdSet &s : g->yd_sets)
    if (s.seq == seq) { mine = &s; break; }
  if (!mine) return MI355_OK;
  const hipEvent_t ev = mine->done;
  mine->waiters++;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  for (YdSet &s : g->yd_sets)
    if (s.seq == seq) { s.waiters--; break; }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipEventSynchronize(group decoder set)"); }
  for (YdSet &s : g->yd_sets)
    if (s.seq <= seq) yd_collect(g, s);
  yd_retire(g);
  return MI355_OK;
}

// waits for every set launched so far (their results stay collectable)
int yd_wait_all_unlocking(mi355_group *g, std::unique_lock<std::mutex> &lk) {
  uint64_t last = 0;
  for (const YdSet &s : g->yd_sets)
    if (!s.collected) last = s.slots.front().ticket;
  return last ? yd_wait_unlocking(g, lk, last) : MI355_OK;
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
  if (g->actx) {
    // pairs still pending are launched and waited for: their frames belong to callers who may free them once this returns
    {
      Locked L(g);
      (void)cmp_flush_locked(g);
    }
    for (int l = 0; l < kCmpMaxLanes; l++)
      if (g->alane[l]) (void)hipStreamSynchronize(g->alane[l]->stream);
    for (CmpBatch &b : g->cmp_batches) { (void)hipEventDestroy(b.done); (void)hipHostFree(b.h_block); }
    g->cmp_batches.clear();
    for (void *b : g->cmp_blocks) (void)hipHostFree(b);
    for (int l = 0; l < kCmpMaxLanes; l++) {
      if (g->d_hash_sums[l]) (void)hipFree(g->d_hash_sums[l]);
      if (g->alane[l]) mi355_ctx_destroy(g->alane[l]);
    }
  }
  if (g->cd_stream) {
    // frames still pending are launched and waited for, as pairs are
    {
      Locked L(g);
      (void)cd_flush_locked(g);
    }
    (void)hipStreamSynchronize(g->cd_stream);
    for (CdSet &s : g->cd_sets) { (void)hipEventDestroy(s.done); (void)hipHostFree(s.h_block); }
    g->cd_sets.clear();
    for (CdDesc &d : g->cd_pending)
      if (d.ready) (void)hipEventDestroy(d.ready);
    g->cd_pending.clear();
    colordetect_set_scratch_free(g->cd_scratch);
    (void)hipStreamDestroy(g->cd_stream);
  }
  for (void *b : g->cd_blocks) (void)hipHostFree(b);
  if (g->hd_stream) {
    // frames still pending are launched and waited for, as pairs are: their destinations are complete when destroy returns
    {
      Locked L(g);
      (void)hd_flush_locked(g);
    }
    (void)hipStreamSynchronize(g->hd_stream);
    for (HdSet &s : g->hd_sets) (void)hipEventDestroy(s.done);
    g->hd_sets.clear();
    for (HdDesc &d : g->hd_pending)
      if (d.ready) (void)hipEventDestroy(d.ready);
    g->hd_pending.clear();
    (void)hipStreamDestroy(g->hd_stream);
  }
  if (g->yd_stream) {
    // tensors still pending are launched and waited for, as frames are: nothing reads a member's tensor once destroy has returned
    if (g->yd_scratch) {
      Locked L(g);
      (void)yd_flush_locked(g);
    }
    (void)hipStreamSynchronize(g->yd_stream);
    for (YdSet &s : g->yd_sets) {
      (void)hipEventDestroy(s.done);
      if (s.block.h) (void)hipHostFree(s.block.h);
    }
    g->yd_sets.clear();
    for (YdDesc &d : g->yd_pending)
      if (d.ready) (void)hipEventDestroy(d.ready);
    g->yd_pending.clear();
    yolodec_set_scratch_free(g->yd_scratch);
    (void)hipStreamDestroy(g->yd_stream);
  }
  for (YdBlock &b : g->yd_blocks) (void)hipHostFree(b.h);
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
  // The frame starts after what ctx's stream holds now (an upload, the table build). A stream that holds nothing - the common
  // case for a stream that only ever submits here - needs no event: every cross-stream wait is a barrier packet the command
  // processor resolves in microseconds, eight of them in front of a 90 us launch are a bubble.
  d.ready = nullptr;
  if (hipStreamQuery(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    d.ready = take_event(g);
    if (!d.ready || hipEventRecord(d.ready, ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (d.ready) g->events.push_back(d.ready);
      return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
    }
  }
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
  const int rc = flush_locked(g);
  const int rc2 = g->actx ? cmp_flush_locked(g) : MI355_OK;
  const int rc3 = g->cd_scratch ? cd_flush_locked(g) : MI355_OK;
  const int rc4 = g->hd_stream ? hd_flush_locked(g) : MI355_OK;
  const int rc5 = g->yd_scratch ? yd_flush_locked(g) : MI355_OK;
  return rc ? rc : (rc2 ? rc2 : (rc3 ? rc3 : (rc4 ? rc4 : rc5)));
}

// ---------------------------------------------------------------- videocompare pairs (Dssim / Blockhash) of independent elements

int mi355_group_set_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  if (!g || expected_streams < 0) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  g->expected_streams = expected_streams;
  g->linger_us = linger_us;
  return MI355_OK;
}

int mi355_group_set_compare_lanes(mi355_group *g, int lanes) {
  if (!g || lanes < 1 || lanes > kCmpMaxLanes) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (g->actx) return fail(g, MI355_ERR_INVALID_ARG, "group: the compare queue's streams exist already (set the lanes before the first submit_compare)");
  g->n_lanes = lanes;
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
  if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  if (!g->actx) {
    int st = MI355_OK;
    for (int l = 0; l < g->n_lanes && !st; l++) {
      g->alane[l] = mi355_ctx_create(g->device, &st);
      if (!g->alane[l] && !st) st = MI355_ERR_HIP;
      if (!st && hipMalloc((void **)&g->d_hash_sums[l], (size_t)2 * kCmpMaxBatch * (64 * 4 + 8)) != hipSuccess) { (void)hipGetLastError(); st = MI355_ERR_OUT_OF_MEMORY; }
    }
    if (st) {
      for (int l = 0; l < kCmpMaxLanes; l++) {
        if (g->d_hash_sums[l]) (void)hipFree(g->d_hash_sums[l]);
        if (g->alane[l]) mi355_ctx_destroy(g->alane[l]);
        g->d_hash_sums[l] = nullptr; g->alane[l] = nullptr;
      }
      return fail(g, st, "group: no contexts for the compare queue");
    }
    g->actx = g->alane[0];
  }
  cmp_retire_done(g);
  CmpDesc d{};
  d.ctx = ctx; d.ref = d_ref; d.frame = d_frame; d.width = width; d.height = height; d.stride = stride; d.format = format; d.algo = algo;
  d.translucent = ctx->dssim_translucent;
  d.fast = ctx->dssim_fast;
  d.ready = nullptr;
  if (hipStreamQuery(ctx->stream) != hipSuccess) {   // the pair starts after what the stream's own context holds now (an upload)
    (void)hipGetLastError();
    d.ready = take_event(g);
    if (!d.ready || hipEventRecord(d.ready, ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (d.ready) g->events.push_back(d.ready);
      return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
    }
  }
  d.ticket = g->next_ticket++;
  if (ticket) *ticket = d.ticket;
  g->cmp_pending.push_back(d);
  // everybody is here (rendezvous), or a launch set is full: go. The pair has been accepted whatever that launch does (a failure
  // is told to the waits of the pairs it carried).
  const int full = g->expected_streams > 0 && g->expected_streams < kCmpMaxBatch ? g->expected_streams : kCmpMaxBatch;
  if ((int)g->cmp_pending.size() >= full) (void)cmp_flush_locked(g);
  return MI355_OK;
}

int mi355_group_wait_compare(mi355_group *g, uint64_t ticket, double *distance, uint64_t hashes[2]) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (ticket == 0 || ticket >= g->next_ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: unknown ticket");
  if (cd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a colordetect frame's ticket (mi355_group_wait_colordetect collects it)");
  if (hd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a hsvdetector frame's ticket (mi355_group_wait_hsvdetect collects it)");
  if (yd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a decoder tensor's ticket (mi355_group_wait_yolodec collects it)");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  auto is_pending = [&]() { for (const CmpDesc &d : g->cmp_pending) if (d.ticket == ticket) return true; return false; };
  if (is_pending()) {
    // rendezvous: the other streams of this interval are about to submit - linger for them (bounded), then launch what is there
    if (g->expected_streams > 0 && g->linger_us > 0) {
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(g->linger_us);
      while (is_pending() && (int)g->cmp_pending.size() < g->expected_streams) {
        if (g->cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
    }
    if (is_pending()) (void)cmp_flush_locked(g, ticket);   // (a failure of this pair's own launch is in cmp_results)
  }
  int rc = cmp_wait_unlocking(g, lk, ticket);
  if (rc) return rc;
  auto r = g->cmp_results.find(ticket);
  if (r == g->cmp_results.end()) return fail(g, MI355_ERR_INVALID_ARG, "group: this pair's result has been collected already (or the ticket is not a pair's)");
  const CmpResult res = r->second;
  g->cmp_results.erase(r);
  if (res.status) return fail(g, res.status, "group: the launch that carried this pair failed");
  if (distance) *distance = res.distance;
  if (hashes) { hashes[0] = res.hashes[0]; hashes[1] = res.hashes[1]; }
  return MI355_OK;
}

int mi355_group_compare_stats(mi355_group *g, uint64_t stats[3]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_cmp_pairs;
  stats[1] = g->n_cmp_batches;
  stats[2] = g->n_cmp_largest;
  return MI355_OK;
}

// ---------------------------------------------------------------- colordetect frames of independent elements

int mi355_group_set_colordetect_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  if (!g || expected_streams < 0) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  g->cd_expected = expected_streams;
  g->cd_linger_us = linger_us;
  return MI355_OK;
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
  if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  if ((rc = cd_ensure(g))) return rc;
  cd_retire_done(g);
  CdDesc d{};
  d.f = CdFrame{d_data, data_len, format, quality, max_colors};
  d.ready = nullptr;
  if (hipStreamQuery(ctx->stream) != hipSuccess) {   // the frame is read after what the context's stream holds now (an upload, a filter)
    (void)hipGetLastError();
    d.ready = take_event(g);
    if (!d.ready || hipEventRecord(d.ready, ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (d.ready) g->events.push_back(d.ready);
      return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
    }
  }
  d.ticket = g->next_ticket++;
  *ticket = d.ticket;
  g->cd_pending.push_back(d);
  // everybody is here (rendezvous), or a launch set is full: go. The frame has been accepted whatever that launch does (a failure
  // is told to the waits of the frames it carried).
  const int full = g->cd_expected > 0 && g->cd_expected < kCdSetMax ? g->cd_expected : kCdSetMax;
  if ((int)g->cd_pending.size() >= full) (void)cd_flush_locked(g);
  return MI355_OK;
}

int mi355_group_wait_colordetect(mi355_group *g, uint64_t ticket, uint8_t palette_rgb[255 * 3], int *n_colors) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (!palette_rgb || !n_colors) return fail(g, MI355_ERR_INVALID_ARG, "group: null result arrays");
  // a filter frame's, a pair's, a detector frame's, a decoder tensor's, a collected or an unknown ticket: refused before anything is launched or waited for
  if (!cd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: not the ticket of a colordetect frame that is still to be collected");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  auto is_pending = [&]() { for (const CdDesc &d : g->cd_pending) if (d.ticket == ticket) return true; return false; };
  if (is_pending()) {
    // rendezvous: the other instances of this interval are about to submit - linger for them (bounded), then launch what is there
    if (g->cd_expected > 0 && g->cd_linger_us > 0) {
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(g->cd_linger_us);
      while (is_pending() && (int)g->cd_pending.size() < g->cd_expected) {
        if (g->cd_cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
    }
    if (is_pending()) (void)cd_flush_locked(g, ticket);   // (a failure of this frame's own launch is in cd_results)
  }
  int rc = cd_wait_unlocking(g, lk, ticket);
  if (rc) return rc;
  auto r = g->cd_results.find(ticket);
  if (r == g->cd_results.end()) return fail(g, MI355_ERR_INVALID_ARG, "group: this frame's palette has been collected already");   // (by a concurrent wait)
  const CdOut res = r->second;
  g->cd_results.erase(r);
  if (res.status) return fail(g, res.status, "group: the launch that carried this colordetect frame failed");
  std::memcpy(palette_rgb, res.rgb, sizeof(res.rgb));
  *n_colors = res.n_colors;
  return MI355_OK;
}

int mi355_group_colordetect_stats(mi355_group *g, uint64_t stats[4]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_cd_frames;
  stats[1] = g->n_cd_sets;
  stats[2] = g->n_cd_largest;
  stats[3] = g->n_cd_launches;
  return MI355_OK;
}

// ---------------------------------------------------------------- hsvdetector frames of independent elements

int mi355_group_set_hsvdetect_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  if (!g || expected_streams < 0) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  g->hd_expected = expected_streams;
  g->hd_linger_us = linger_us;
  return MI355_OK;
}

int mi355_group_submit_hsvdetect(mi355_group *g, mi355_ctx *ctx, const uint8_t *d_src, int src_stride, int src_format, uint8_t *d_dst, int dst_stride,
                                 int dst_format, int width, int height, const mi355_hsvdetect_settings *settings, uint64_t *ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  if (!ctx || !ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: null context or ticket");
  HdDesc d{};
  const char *why = nullptr;
  int rc = hsvdetect_check_frames(d_src, src_stride, src_format, d_dst, dst_stride, dst_format, 1, width, height, settings, &d.f.sfmt, &d.f.dst_alpha_first,
                                  &d.f.dst_bgr, &why);
  if (rc) return fail(g, rc, why);
  if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  if ((rc = hd_ensure(g))) return rc;
  hd_retire_done(g);
  d.f.src = d_src;
  d.f.dst = d_dst;
  d.f.src_stride = src_stride;
  d.f.dst_stride = dst_stride;
  d.f.width = width;
  d.f.height = height;
  d.f.s = *settings;
  d.f.force_generic = ctx->force_generic;
  d.ready = nullptr;
  if (width > 0 && height > 0 && hipStreamQuery(ctx->stream) != hipSuccess) {   // the frame is read after what the context's stream holds now (an upload, a filter)
    (void)hipGetLastError();
    d.ready = take_event(g);
    if (!d.ready || hipEventRecord(d.ready, ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (d.ready) g->events.push_back(d.ready);
      return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
    }
  }
  d.ticket = g->next_ticket++;
  *ticket = d.ticket;
  g->hd_pending.push_back(d);
  // everybody is here (rendezvous), or a launch set is full: go. The frame has been accepted whatever that launch does (a failure
  // is told to the waits of the frames it carried).
  const int full = g->hd_expected > 0 && g->hd_expected < kHdSetMax ? g->hd_expected : kHdSetMax;
  if ((int)g->hd_pending.size() >= full) (void)hd_flush_locked(g);
  return MI355_OK;
}

int mi355_group_wait_hsvdetect(mi355_group *g, uint64_t ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  // another queue's, a collected or an unknown ticket: refused before anything is launched or waited for
  if (!hd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: not the ticket of a hsvdetector frame that is still to be collected");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  auto is_pending = [&]() { for (const HdDesc &d : g->hd_pending) if (d.ticket == ticket) return true; return false; };
  if (is_pending()) {
    // rendezvous: the other instances of this interval are about to submit - linger for them (bounded), then launch what is there
    if (g->hd_expected > 0 && g->hd_linger_us > 0) {
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(g->hd_linger_us);
      while (is_pending() && (int)g->hd_pending.size() < g->hd_expected) {
        if (g->hd_cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
    }
    if (is_pending()) (void)hd_flush_locked(g, ticket);   // (a failure of this frame's own launch is in hd_results)
  }
  int rc = hd_wait_unlocking(g, lk, ticket);
  if (rc) return rc;
  auto r = g->hd_results.find(ticket);
  if (r == g->hd_results.end()) return fail(g, MI355_ERR_INVALID_ARG, "group: this frame has been collected already");   // (by a concurrent wait)
  const int status = r->second;
  g->hd_results.erase(r);
  if (status) return fail(g, status, "group: the launch that carried this hsvdetector frame failed");
  return MI355_OK;
}

int mi355_group_hsvdetect_stats(mi355_group *g, uint64_t stats[4]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_hd_frames;
  stats[1] = g->n_hd_sets;
  stats[2] = g->n_hd_largest;
  stats[3] = g->n_hd_launches;
  return MI355_OK;
}

int mi355_selftest_hsvdetect_plan(int n_cu, int blocks_per_cu, unsigned units_per_block, int n_jobs, const uint64_t *units, uint32_t *first_block,
                                  uint32_t *blocks, uint32_t *total_blocks) {
  return hsvdetect_plan(n_cu, blocks_per_cu, units_per_block, n_jobs, units, first_block, blocks, total_blocks);
}

// ---------------------------------------------------------------- decoder tensors of independent elements

int mi355_group_set_yolodec_rendezvous(mi355_group *g, int expected_streams, unsigned linger_us) {
  if (!g || expected_streams < 0) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  g->yd_expected = expected_streams;
  g->yd_linger_us = linger_us;
  return MI355_OK;
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
  if (ctx->device != g->device) return fail(g, MI355_ERR_INVALID_ARG, "group: context of another device");
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  if ((rc = yd_ensure(g))) return rc;
  yd_retire_done(g);
  YdDesc d{};
  d.t = YdTensor{d_tensor, layout, num_fields, num_candidates, max_dets, *p};
  d.ready = nullptr;
  if (num_candidates && hipStreamQuery(ctx->stream) != hipSuccess) {   // the tensor is read after what the context's stream holds now (an upload, the model's last kernel)
    (void)hipGetLastError();
    d.ready = take_event(g);
    if (!d.ready || hipEventRecord(d.ready, ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (d.ready) g->events.push_back(d.ready);
      return fail(g, MI355_ERR_HIP, "group: hipEventRecord(ready)");
    }
  }
  d.ticket = g->next_ticket++;
  *ticket = d.ticket;
  g->yd_pending.push_back(d);
  // everybody is here (rendezvous), or a launch set is full: go. The tensor has been accepted whatever that launch does (a failure
  // is told to the waits of the tensors it carried).
  const int full = g->yd_expected > 0 && g->yd_expected < kYdSetMax ? g->yd_expected : kYdSetMax;
  if ((int)g->yd_pending.size() >= full) (void)yd_flush_locked(g);
  return MI355_OK;
}

int mi355_group_wait_yolodec(mi355_group *g, uint64_t ticket, mi355_yolo_det *dets, uint32_t *n_dets) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (!n_dets) return fail(g, MI355_ERR_INVALID_ARG, "group: null result count");
  // another queue's, a collected or an unknown ticket: refused before anything is launched or waited for
  if (!yd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: not the ticket of a decoder tensor that is still to be collected");
  if (!dets) {   // only a tensor submitted with max_dets == 0 has no records to take
    uint32_t cap = 0;
    for (const YdDesc &d : g->yd_pending)
      if (d.ticket == ticket) cap = d.t.max_dets;
    auto w = g->yd_where.find(ticket);
    if (w != g->yd_where.end())
      for (const YdSet &s : g->yd_sets)
        if (s.seq == w->second)
          for (const YdSlot &sl : s.slots)
            if (sl.ticket == ticket) cap = sl.max_dets;
    auto r = g->yd_results.find(ticket);
    if (r != g->yd_results.end()) cap = r->second.max_dets;
    if (cap) return fail(g, MI355_ERR_INVALID_ARG, "group: null records for a tensor submitted with max_dets > 0");
  }
  if (hipSetDevice(g->device) != hipSuccess) { (void)hipGetLastError(); return fail(g, MI355_ERR_HIP, "hipSetDevice"); }
  auto is_pending = [&]() { for (const YdDesc &d : g->yd_pending) if (d.ticket == ticket) return true; return false; };
  if (is_pending()) {
    // rendezvous: the other instances of this interval are about to submit - linger for them (bounded), then launch what is there
    if (g->yd_expected > 0 && g->yd_linger_us > 0) {
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(g->yd_linger_us);
      while (is_pending() && (int)g->yd_pending.size() < g->yd_expected) {
        if (g->yd_cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
    }
    if (is_pending()) (void)yd_flush_locked(g, ticket);   // (a failure of this tensor's own launch is in yd_results)
  }
  int rc = yd_wait_unlocking(g, lk, ticket);
  if (rc) return rc;
  auto r = g->yd_results.find(ticket);
  if (r == g->yd_results.end()) return fail(g, MI355_ERR_INVALID_ARG, "group: this tensor's result has been collected already");   // (by a concurrent wait)
  const YdOut res = std::move(r->second);
  g->yd_results.erase(r);
  if (res.status) return fail(g, res.status, "group: the launch that carried this decoder tensor failed");
  *n_dets = res.n_dets;
  if (dets && !res.dets.empty()) std::memcpy(dets, res.dets.data(), res.dets.size() * sizeof(mi355_yolo_det));
  return MI355_OK;
}

int mi355_group_yolodec_stats(mi355_group *g, uint64_t stats[4]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_yd_tensors;
  stats[1] = g->n_yd_sets;
  stats[2] = g->n_yd_largest;
  stats[3] = g->n_yd_launches;
  return MI355_OK;
}

int mi355_group_wait(mi355_group *g, uint64_t ticket) {
  if (!g) return MI355_ERR_INVALID_ARG;
  Locked L(g);
  std::unique_lock<std::mutex> &lk = L.lk;
  if (ticket == 0 || ticket >= g->next_ticket) return fail(g, MI355_ERR_INVALID_ARG, "group: unknown ticket");
  if (cd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a colordetect frame's ticket (mi355_group_wait_colordetect collects it)");
  if (hd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a hsvdetector frame's ticket (mi355_group_wait_hsvdetect collects it)");
  if (yd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a decoder tensor's ticket (mi355_group_wait_yolodec collects it)");
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
  if (cd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a colordetect frame's ticket (mi355_group_wait_colordetect collects it)");
  if (hd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a hsvdetector frame's ticket (mi355_group_wait_hsvdetect collects it)");
  if (yd_owns(g, ticket)) return fail(g, MI355_ERR_INVALID_ARG, "group: a decoder tensor's ticket (mi355_group_wait_yolodec collects it)");
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
  if (g->cd_scratch) {
    if ((rc = cd_flush_locked(g))) return rc;
    if ((rc = cd_wait_all_unlocking(g, lk))) return rc;
  }
  if (g->hd_stream) {
    if ((rc = hd_flush_locked(g))) return rc;
    if ((rc = hd_wait_all_unlocking(g, lk))) return rc;
  }
  if (!g->yd_scratch) return MI355_OK;
  if ((rc = yd_flush_locked(g))) return rc;
  return yd_wait_all_unlocking(g, lk);
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
