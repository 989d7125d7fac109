// ctx.hpp — what the host translation units (capi*.cpp, stream_*.cpp) share and no kernel sees: the context, the one
// type that owns device or pinned memory, the error helpers (fail, HIP_TRY, MD_LAUNCH_TRY), the device guard of the entry
// points, the carving of a scratch block into arrays (md::Carver of host_util.hpp, carve), and every function that
// one of those files defines and another calls.  The defining file and every caller include it, as with internal.hpp.
// Plain host C++.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "host_util.hpp"
#include "internal.hpp"
#include "mdeflate.h"

// nothing here is exported but the extern "C" functions below
#pragma GCC visibility push(hidden)

// records `what` (and HIP's text for e) as the last error of ctx and of the calling thread, returns code.  ONE definition
// (capi.cpp, beside the thread's string that md_last_error_string(NULL) reads).
int fail(md_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess);

#define HIP_TRY(ctx, expr)                                   \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) return fail(ctx, MD_E_HIP, #expr, e_); \
  } while (0)

// the same for a launcher of internal.hpp, which returns HIP's error as an int
#define MD_LAUNCH_TRY(ctx, expr)                                    \
  do {                                                              \
    const int e_ = (expr);                                          \
    if (e_ != 0) return fail(ctx, MD_E_HIP, #expr, (hipError_t)e_); \
  } while (0)

#define MD_ON_DEVICE(ctx)                 \
  md::DeviceGuard guard_((ctx)->device);  \
  if (!guard_.ok) return fail(ctx, MD_E_HIP, "hipSetDevice")

namespace md {

// every entry point works on the context's device and leaves the caller's current device as it found it
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    if (!ok) (void)hipGetLastError();  // (the call reports the failure itself: no stale error for whoever asks next)
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// most input that one src call of a streaming encoder, or one round of a decoder of a batch, hands over: positions
// within a launch are 32-bit
constexpr size_t kSrcMax = (size_t)1 << 30;

// what the batch shims ask of the allocator for a blob of `need` bytes: a quarter and 4 KiB of headroom
inline size_t blob_room(size_t need) { return need + need / 4 + 4096; }

// md_set_option "zip_crc_segment" = 0: the lowest median of 64 KiB .. 1 MiB for one stored entry of 1 GiB, alone and beside
// 2 464 deflated ones (all five within 1 % of each other) - 4 096 wavefronts for 1 GiB, 16 a CU
constexpr size_t kZipSegmentDefault = (size_t)256 << 10;

// md_set_option "deflate_span_kib" = 0: text per span of md_deflate_spans_*.  The largest of 64 KiB .. 1 MiB whose time for
// 64 MiB is within 10 % of the fastest, on text and on random bytes (51.9 ms; 128 KiB takes 57.4 ms on text)
constexpr size_t kSpanDefault = (size_t)64 << 10;

// One allocation of device (or pinned host) memory and its capacity.  It frees itself when its owner goes: whoever
// deletes the owner sets the device and waits for the context's stream first.  Grow-only, and growing does not keep the
// contents (reserve_keep does).
template <bool kPinned>
struct Buffer {
  void *p = nullptr;
  size_t cap = 0;
  Buffer() = default;
  Buffer(const Buffer &) = delete;
  Buffer &operator=(const Buffer &) = delete;
  Buffer(Buffer &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buffer &operator=(Buffer &&o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~Buffer() { release(); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const {
    return (T *)p;
  }
  // Nothing when `need` bytes are there.  Otherwise the context's stream is waited for, the block is freed and `room`
  // bytes are allocated (`need` itself unless the caller asks for headroom); no room: MD_E_OUT_OF_MEMORY, with `what` as
  // the context's error text unless it is null (the batch shims report the status alone).
  int reserve(md_ctx *ctx, size_t need, const char *what, size_t room = 0);
  int reserve_blob(md_ctx *ctx, size_t need) { return reserve(ctx, need, nullptr, blob_room(need)); }
  // a blob (device) that keeps its first `keep` bytes when it grows
  int reserve_keep(md_ctx *ctx, size_t need, size_t keep);
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// The device's time for a stretch of the context's stream: begin and end record the two events around it.  A call that
// waits for the stream reads ns() behind its synchronise; one that reads nothing back sets `pending`, and whoever asks for
// the time later settles it.  md_create makes the events, md_destroy frees them.
struct EventSpan {
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool pending = false;
  hipError_t begin(hipStream_t st) { return hipEventRecord(ev[0], st); }
  hipError_t end(hipStream_t st) { return hipEventRecord(ev[1], st); }
  // behind a synchronise (an event that cannot be read leaves 0)
  uint64_t ns() const {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) ms = 0, (void)hipGetLastError();
    return (uint64_t)((double)ms * 1e6);
  }
  // a pending time into *out, behind a wait for the end event; nothing when none is pending
  hipError_t settle(uint64_t *out) {
    if (!pending) return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev[1]);
    if (e != hipSuccess) return e;
    *out = ns();
    pending = false;
    return hipSuccess;
  }
};

// pairs of events around a step that a call repeats - the apply launches of a read's rounds (md_pack_stats::apply_ns), the
// hash passes (md_sha1_stats::device_ns), the link passes and the steps of a walk (capi_pack_graph.cpp); an event that
// cannot be had leaves the time 0, never fails the call
struct PairTimers {
  std::vector<hipEvent_t> ev;
  void mark(hipStream_t st) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) e = nullptr, (void)hipGetLastError();
    if (e && hipEventRecord(e, st) != hipSuccess) (void)hipGetLastError();
    ev.push_back(e);
  }
  uint64_t total_ns() const {  // (behind a synchronise of the stream)
    double ms = 0;
    for (size_t k = 0; k + 1 < ev.size(); k += 2) {
      float t = 0;
      if (ev[k] && ev[k + 1] && hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) ms += t;
      else (void)hipGetLastError();
    }
    return (uint64_t)(ms * 1e6);
  }
  ~PairTimers() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace md

// The context's grow-only scratch.  md_set_option "release_workspace" gives back exactly these, in this order (they grow
// again on demand); gz_tmp, lzo_ws, counters, dbg and gz_hdr_dev below are not among them and live as long as the context.
enum Scratch {
  // deflate: command queues (n x queue_len), the per-stream part of the front workspace (slots, chunk starts: n-sized)
  // and its per-position part (hash-chain links, look-ahead verdicts: 13 bytes per input byte)
  kWs, kFsmall, kFbig,
  kOrder,  // launch order of a large batch (4 bytes per stream)
  // the decoder in pieces (md_de_inf_continue_host): input, output and descriptors
  kContIn, kContOut, kContDesc,
  // a deflate batch in slices of positions: descriptors of the slice and the streams' states between the slices
  kSliceDesc, kSliceState,
  // the host-buffer entry points (md_*_batch_host): device copies of the caller's blobs and descriptors
  kHostIn, kHostOut, kHostDesc,
  // one long stream decoded by the whole chip (inflate_parallel): input, output + the pieces' scratch decodes, windows
  // and descriptors
  kParIn, kParOut, kParWin, kParDesc,
  // a GZip file of many members (md_gz_members_*, md_bgzf_compress): the member scan's bitmap and counts, its candidate
  // lists, the members' descriptors, and the writer's packed file (the reader of a file without size fields decodes its
  // batch into that one: its host steps go through kHostIn / kHostOut)
  // (md_deflate_spans_*: descriptors in kGzmDesc, the joined stream of the host form in kGzmOut, slots in kHostOut)
  // (md_pack_index_build: the candidates' bitmap and counts in kGzmWs, their list in kGzmCand, the size query's arrays in kGzmDesc)
  kGzmWs, kGzmCand, kGzmDesc, kGzmOut,
  // a ZIP archive (md_zip_*): rows, names, descriptors and the segment table; the writer's file image (archive bytes and
  // decoded entries / encoder slots go through kHostIn / kHostOut)
  kZipDesc, kZipOut,
  // the index of a long stream (md_inflate_index_*): compressed bytes of the pieces of a round, the pieces' slots (window +
  // output), windows on their way in (read) or out (build), tables and descriptors, the ranges' bytes
  kZixIn, kZixSlots, kZixWin, kZixDesc, kZixOut,
  // byte ranges of a blocked GZip file (md_bgzf_read): the touched members of a round packed back to back, their output
  // slots (tables and descriptors go through kGzmDesc, the ranges' bytes through kHostOut)
  kBgrIn, kBgrSlots,
  // a git packfile (md_pack_*): the table of md_pack_open, the descriptors of a round, the delta payloads of md_pack_open (the
  // pack goes through kHostIn; a read's output and its round's scratch are one block, kHostOut)
  kPackDesc, kPackRound, kPackScratch,
  // SHA-1 of many messages (md_sha1_batch_*, the names of a round of md_pack_read / md_pack_verify): descriptors, states
  // and digests (the host form's bytes go through kHostIn)
  kShaDesc,
  // a delta plan on the device (md_pack_delta_batch_*, md_pack_delta_sizes_*, the deltas of md_pack_write, the scores of
  // md_pack_choose_bases): pairs, bases and - unless they are the caller's - the results in kPkwDesc; the bases' tables.
  // Writing a pack: the per-object arrays, the compressed payloads (the objects and behind them the deltas stand in
  // kHostIn, the pack in kHostOut).  Sketches (md_pack_sketch_*, md_pack_choose_bases): segments and features in kPkwDesc,
  // in front of the plan that md_pack_choose_bases puts there next; the objects in kHostIn
  kPkwDesc, kPkwTables, kPkwObjs, kPkwSlots,
  // the object graph of a pack (md_pack_graph_build): the names, fan-out and types the link kernels look up in, the slots'
  // offsets, the edge counts and the malformed flags in kPkgDesc, the bound-sized edge slots in kPkgSlots (the compacted
  // edges are the graph's own).  md_pack_reachable: marks, frontiers, seeds and the result in kPkgDesc
  kPkgDesc, kPkgSlots,
  // trees diffed (md_pack_diff): a level's descriptors, tables of entries, counts and places in kPkdDesc, its records and their
  // names in kPkdOut (the level's trees stand in kHostOut, where the read left them)
  kPkdDesc, kPkdOut,
  kScratchCount
};

// The table of a pack, all of it on the host: a read uploads the rows of the objects it needs.
struct md_pack {
  uint64_t pack_len = 0;
  md_pack_info info = {};
  uint8_t pack_checksum[20] = {0};
  uint32_t fan[256] = {0};
  std::vector<md_pack_object> objs;  // idx order (md_pack_index_build's own tables: pack order)
  std::vector<uint64_t> zoff, hsize;  // where an object's zlib stream begins, the size its header states
  std::vector<uint32_t> crc;          // the idx's CRC-32 of the packed object
  std::vector<uint8_t> delta;         // 1: the object is a delta (with a base in the pack)
};

struct md_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  md::EventSpan timing;  // md_timing_begin / md_timing_end
  md::DevBuf scratch[kScratchCount];
  // GZip: per-stream scratch (body_off[n], body_len[n] u64, hstatus[n] i32, crc[n] u32), grow-only, and the header to write
  md::DevBuf gz_tmp;
  md::DevBuf gz_hdr_dev;           // device copy of gz_hdr (530 bytes max)
  uint8_t gz_hdr_sent[544] = {0};  // what gz_hdr_dev holds
  bool gz_hdr_valid = false;
  md::DevBuf lzo_ws;    // Lzo.compress dictionaries
  md::DevBuf counters;  // work counters of the kernels with persistent workgroups (zeroed in front of a launch)
  int cus = 256;        // compute units of the device
  int inflate_waves = 2;    // wavefronts per stream of the inflate kernel (md_set_option "inflate_waves": 1 = the one-wavefront form)
  size_t piece_bytes = (size_t)1 << 20;  // md_set_option "encoder_piece_bytes": input the md_def_* encoder gathers before a launch
  size_t front_cap_bytes = 0;  // md_set_option "deflate_workspace_cap_mib" (md_create: a sixth of the device's memory; 0 = none):
                               // batches whose per-position workspace would be larger go in slices of positions
  int test_flags = 0;  // md_set_option "deflate_test_flags": bit 4 = the md_def_* encoder moves its origin every 128 KiB (tests),
                       // bit 5 = the match kernel also takes the chunks below SeqArgs::first (primed spans; a measurement)
  md::DevBuf dbg;      // device buffer of the optional in-kernel profile (32 x u64)
  // the two copy streams of the host-buffer entry points, next to the context's stream (copy-in of slice k + 1 and
  // copy-out of slice k - 1 under the kernels of slice k)
  hipStream_t s_in = nullptr, s_out = nullptr;
  // one long stream by the whole chip: md_set_option "inflate_parallel_min" (compressed bytes from which a single stream
  // goes this way, 0 = never) and "inflate_parallel_chunk" (compressed bytes per piece)
  size_t par_min = (size_t)96 << 10, par_chunk = (size_t)64 << 10;  // (measured: the pieces pay from ~100 KB of input, ~1 ms flat up to 4 MiB of text)
  int par_last_pieces = 0, par_last_rounds = 0;  // of the last stream that went this way (md_get_option, tests)
  int host_slices_max = 16;  // md_set_option "host_pipeline_slices": 1 = copy-in / kernels / copy-out one after the other
  // ONE long stream's hash chains in segments on the whole chip (link_segments): md_set_option
  // "deflate_link_segment_min" (input bytes from which a single stream of md_deflate_batch_host goes this way, 0 = never)
  // and "deflate_link_segment" (positions per segment, 0 = by the stream's length); link_last_segments: the segments
  // the last deflate batch call built its chains in (0 = one workgroup per stream; md_i_link_segments, tests)
  size_t link_seg_min = (size_t)128 << 10, link_seg = 0;
  uint32_t link_last_segments = 0;
  // a GZip file of many members without size fields: md_set_option "gz_members_speculate" (0 = member by member on the
  // host, as before there was a speculative path), and which way the last md_gz_members_uncompress went (md_gz_members_last)
  bool gzm_speculate = true;
  md_gz_members_stats gzm_last = {};
  // ZIP archives: md_set_option "zip_crc_segment", bytes of an entry's output per wavefront of the copy-and-checksum kernel
  size_t zip_segment = md::kZipSegmentDefault;
  // the index of a long stream: md_set_option "index_read_workspace" (bytes of piece scratch per round of a read; 0 = one
  // piece a round) and the counts of the last md_inflate_index_read (md_inflate_index_last)
  size_t zix_workspace = (size_t)256 << 20;
  md_inflate_index_stats zix_last = {};
  // byte ranges of a blocked GZip file: md_set_option "bgzf_read_workspace" (bytes of packed input and output slots per
  // round of md_bgzf_read; 0 = one member a round) and the counts of the last read (md_bgzf_read_last)
  size_t bgr_workspace = (size_t)256 << 20;
  md_bgzf_read_stats bgr_last = {};
  // git packfiles: md_set_option "pack_workspace" (bytes of scratch per round of md_pack_open / md_pack_read; 0 = one selected
  // object a round) and the counts of the last md_pack_read (md_pack_last)
  size_t pack_workspace = (size_t)256 << 20;
  md_pack_stats pack_last = {};
  md_pack_build_stats pack_build_last = {};  // of the last md_pack_index_build (md_pack_build_last)
  // SHA-1 batches: md_set_option "sha1_launch_blocks" (blocks of 64 bytes by which one launch advances a message) and the
  // counts of the last batch (md_sha1_last), with the span around its launches.  The device form reads nothing back: its
  // time is pending until the counts are asked for
  uint32_t sha1_launch_blocks = md::sha::kLaunchBlocksDefault;
  md_sha1_stats sha1_last = {};
  md::EventSpan sha1_span;
  // making deltas and writing packs: the counts of the last md_pack_delta_batch_* / md_pack_delta_sizes_* / md_pack_write
  // (md_pack_write_last) and the span around the index launch and the delta or size launch; the device forms leave it pending.
  // md_pack_choose_bases times its sketch launch and its scores with the same span, one after the other
  md_pack_write_stats pack_write_last = {};
  md::EventSpan pkw_span;
  // choosing bases: the counts and times of the last md_pack_choose_bases (md_pack_search_last)
  md_pack_search_stats pack_search_last = {};
  // walking a pack's graph: the counts and the time of the last md_pack_reachable (md_pack_reach_last)
  md_pack_reach_stats pack_reach_last = {};
  // one stream written as joined spans: md_set_option "deflate_span_kib" (the span of a call that passes 0) and the counts of
  // the last md_deflate_spans_* call (md_deflate_spans_last)
  size_t span_bytes = md::kSpanDefault;
  bool span_prime = false;  // md_set_option "deflate_span_prime": every span is primed with the 32 KiB of text in front of it
  md_deflate_spans_info spans_last = {};
  md::DevBuf spans_count;      // the device word that counts the stored spans of a call
  bool spans_pending = false;  // spans_last.stored_spans is still in spans_count (the device form reads nothing back)
  std::string err;
};

namespace md {

template <bool kPinned>
int Buffer<kPinned>::reserve(md_ctx *ctx, size_t need, const char *what, size_t room) {
  if (need <= cap) return MD_OK;
  if (p) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  if (room < need) room = need;
  if ((kPinned ? hipHostMalloc(&p, room, hipHostMallocDefault) : hipMalloc(&p, room)) != hipSuccess) {
    p = nullptr;
    return what ? fail(ctx, MD_E_OUT_OF_MEMORY, what) : MD_E_OUT_OF_MEMORY;
  }
  cap = room;
  return MD_OK;
}

template <bool kPinned>
int Buffer<kPinned>::reserve_keep(md_ctx *ctx, size_t need, size_t keep) {
  static_assert(!kPinned, "device blobs only");
  if (need <= cap) return MD_OK;
  Buffer q;
  if (hipMalloc(&q.p, blob_room(need)) != hipSuccess) {
    q.p = nullptr;
    return MD_E_OUT_OF_MEMORY;
  }
  q.cap = blob_room(need);
  if (keep) HIP_TRY(ctx, hipMemcpyAsync(q.p, p, keep, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *this = std::move(q);
  return MD_OK;
}

}  // namespace md

// the launch-order scratch of a batch of n streams: null (index order) below `from` streams
inline int launch_order(md_ctx *ctx, size_t n, size_t from, uint32_t **order) {
  *order = nullptr;
  if (n < from) return MD_OK;
  const int rc = ctx->scratch[kOrder].reserve(ctx, n * 4, "hipMalloc(launch order)");
  if (rc == MD_OK) *order = ctx->scratch[kOrder].as<uint32_t>();
  return rc;
}

// A block carved in two passes, the takes written once: `takes` runs over a carver that only counts (null pointers), then
// `buf` is reserved for what it counted and `slack` bytes more, and `takes` runs again over the block.  what == nullptr: no
// error text (Buffer::reserve).
//   rc = carve(ctx, buf, "hipMalloc(..)", [&](md::Carver &c) { a = c.take<uint64_t>(n), b = c.take<int32_t>(n); });
template <class Takes>
int carve(md_ctx *ctx, md::DevBuf &buf, const char *what, Takes takes, size_t slack = 0) {
  md::Carver c;
  takes(c);
  const int rc = buf.reserve(ctx, c.at + slack, what);
  if (rc != MD_OK) return rc;
  c = md::Carver(buf.p);
  takes(c);
  return MD_OK;
}

namespace md {
// count elements between host and device (or count zeroed elements) on st; nothing for a count of 0.  The byte count is
// the type's: HIP_TRY(ctx, md::to_device(d_off, off, n, st)).
template <class T>
hipError_t to_device(T *d, const T *h, size_t count, hipStream_t st) {
  return count ? hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, st) : hipSuccess;
}
template <class T>
hipError_t to_device(T *d, const std::vector<T> &h, hipStream_t st) {
  return to_device(d, h.data(), h.size(), st);
}
template <class T>
hipError_t to_host(T *h, const T *d, size_t count, hipStream_t st) {
  return count ? hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}
template <class T>
hipError_t zero(T *d, size_t count, hipStream_t st) {
  return count ? hipMemsetAsync(d, 0, count * sizeof(T), st) : hipSuccess;
}
}  // namespace md

// f() with the host running out of memory inside it as the context's error `what`
template <class F>
int no_bad_alloc(md_ctx *ctx, const char *what, F f) {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return fail(ctx, MD_E_OUT_OF_MEMORY, what);
  }
}

// the caller's bytes into kHostIn, on the context's stream
inline int upload_host_in(md_ctx *ctx, const uint8_t *src, size_t len) {
  const int rc = ctx->scratch[kHostIn].reserve(ctx, len + 64, "hipMalloc(host path input)");
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_device(ctx->scratch[kHostIn].as<uint8_t>(), src, len, ctx->stream));
  return MD_OK;
}

// the parameters of MD_FORMAT_GZIP (Gz.Def's make_block: Zl driver, dynamic blocks, queue 4096) for the raw body alone, as
// the writers of blocked gzip and of ZIP archives hand them to md_deflate_batch_device with MD_FORMAT_DEFLATE
inline md_deflate_params gzip_body_params(int level, size_t total_in_bytes) {
  md_deflate_params p = {};
  p.level = level;
  p.queue_len = 4096;
  p.driver = MD_DRIVER_ZL;
  p.dynamic = 1;
  p.matcher = MD_MATCHER_DE;
  p.total_in_bytes = total_in_bytes;
  return p;
}

// One host buffer through a batch of one: input, output (16 bytes of slack each: Lzo's compressor over-copies into it)
// and the descriptor (in_off in_len out_off out_cap out_len, status) live for the call; `launch(d_in, d64, d_out,
// d_status, d_extra)` enqueues the batch entry point with n = 1 on the context's stream.  extra_bytes of device memory
// go to the launch as a further result and come back in `extra` when that is not null.  Returns the stream's status.
template <class Launch>
int one_through_batch(md_ctx *ctx, const void *src, size_t src_len, void *dst, size_t dst_cap, size_t *written, Launch launch,
                      size_t extra_bytes = 0, void *extra = nullptr) {
  md::DevBuf din, dout, ddesc, dextra;
  int rc = din.reserve(ctx, src_len + 16, "hipMalloc");
  if (rc == MD_OK) rc = dout.reserve(ctx, dst_cap + 16, "hipMalloc");
  if (rc == MD_OK) rc = ddesc.reserve(ctx, 6 * 8 + 16, "hipMalloc");
  if (rc == MD_OK) rc = dextra.reserve(ctx, extra_bytes, "hipMalloc");
  if (rc != MD_OK) return rc;
  const uint64_t desc[5] = {0, src_len, 0, dst_cap, 0};
  uint64_t *d64 = ddesc.as<uint64_t>();
  int32_t *dstatus = (int32_t *)(d64 + 5);
  hipStream_t st = ctx->stream;
  if (src_len) HIP_TRY(ctx, hipMemcpyAsync(din.p, src, src_len, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d64, desc, sizeof desc, hipMemcpyHostToDevice, st));
  rc = launch(din.as<const uint8_t>(), d64, dout.as<uint8_t>(), dstatus, dextra.as<uint32_t>());
  if (rc != MD_OK) return rc;
  uint64_t out_len = 0;
  int32_t status = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&out_len, d64 + 4, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&status, dstatus, 4, hipMemcpyDeviceToHost, st));
  if (extra) HIP_TRY(ctx, hipMemcpyAsync(extra, dextra.p, extra_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (status == MD_OK && out_len) HIP_TRY(ctx, hipMemcpy(dst, dout.p, (size_t)out_len, hipMemcpyDeviceToHost));
  *written = (size_t)out_len;
  return status;
}

// ---- capi_deflate.cpp: the encoder in pieces, as stream_def.cpp drives it (not part of the public ABI) ----
// The device goes on from the state the piece before left, so neither side keeps more of the stream than the 64 KiB the
// matcher can reach back plus the piece.
struct md_piece;
// one piece of each of n streams, the descriptors host arrays of n entries (md_i_pieces_run)
struct md_pieces_io {
  const uint64_t *text_off, *text_len, *abs_len, *out_off, *out_cap, *w0, *rebase;
  const uint32_t *flags, *sum, *isize;
  uint64_t *out_len;
  int32_t *status;
};

#pragma GCC visibility pop
extern "C" {
int md_validate_deflate_params(md_ctx *ctx, int format, const md_deflate_params *params);
md_piece *md_i_piece_open(md_ctx *ctx, int queue_len);
void md_i_piece_close(md_ctx *ctx, md_piece *p);
int md_i_piece_run(md_ctx *ctx, md_piece *p, int format, const md_deflate_params *params, const uint8_t *text, size_t text_len,
                   size_t seen, uint64_t w0, uint64_t rebase, int first, int last, uint32_t sum, uint32_t isize, size_t out_cap,
                   size_t *out_len, int *status);
int md_i_piece_out(md_ctx *ctx, const md_piece *p, size_t off, uint8_t *host, size_t len);
// d_desc: the caller's, grown here to the n streams' descriptors
int md_i_pieces_run(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_text, uint8_t *d_out,
                    void *d_state, void *d_queue, md::DevBuf &d_desc, const md_pieces_io *io, uint32_t match_skip);
// test hooks that Python binds, and the profile read-back beside md_set_option "profile"
int md_i_link_segments(const md_ctx *ctx);
int md_get_profile(md_ctx *ctx, uint64_t *out32);
}

#pragma GCC visibility push(hidden)
// ---- capi_deflate.cpp ----
// The bytes Gz.Def writes in front of the body for the header fields g (null: the default header); returns the length, 0
// when a field is out of range.
uint32_t gz_header_bytes(const md_gz_header *g, int level, uint8_t h[544]);
// md_deflate_batch_device that also leaves every stream's tail (SeqArgs::tail of internal.hpp: two words per stream) in d_tail;
// d_first: SeqArgs::first (where each stream begins to emit: the text in front of it only primes the matcher), or null
int deflate_batch_tails(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                        const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap, uint64_t *d_out_len,
                        int32_t *d_status, uint32_t *d_checksum, uint64_t *d_tail, const uint32_t *d_first);
// ---- capi_inflate.cpp ----
// One piece of a raw DEFLATE stream through one pair of wavefronts, its output LEFT ON THE DEVICE: src[0, src_len) starts
// start_bit bits into src[0], hist[0, hist_len) is the output in front of it and goes to the start of kContOut, the new
// bytes follow it there, `room` of them at the most.  out_len and resume_out count from the start of kContOut (the window
// included); resume_* say where the last complete block of the piece ended.
struct InfPiece {
  int status;
  uint64_t out_len, consumed, resume_bits, resume_out;
  uint32_t checksum, resume_adler, resume_last;
};
int inflate_piece(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, const uint8_t *hist, size_t hist_len, uint64_t room,
                  uint32_t adler_in, InfPiece *r);
// the same with the output copied out behind the window in dst, and the CRC-32s that flags ask for
int continue_serial(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                    size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status, md_inf_resume *resume);
// ---- capi_gz_members.cpp ----
// the members of an indexed file: device arrays of M entries (out_off: M + 1), carved from ctx->scratch[kGzmDesc].p
struct GzmIndex {
  uint64_t M = 0, total = 0;  // members, the sum of their ISIZE fields
  uint64_t *mpos = nullptr, *mlen = nullptr, *body_off = nullptr, *body_len = nullptr, *isize = nullptr, *out_len = nullptr,
           *consumed = nullptr, *out_off = nullptr, *first = nullptr;
  int32_t *hstatus = nullptr, *status = nullptr;
};
// Mark, chain and descriptors (gz_members.hip) for len bytes at d_src, no decoding.  *indexed: the chain of BC size fields
// leads from offset 0 to the end of the file; then ix holds the members, their headers parsed and their output offsets
// scanned (md_gz_members_scan, md_gz_members_uncompress, md_bgzf_index_build).
int gzm_index(md_ctx *ctx, const uint8_t *d_src, uint64_t len, bool *indexed, GzmIndex *ix);
// ---- capi_sha1.cpp ----
// What a batch of n messages keeps on the device, carved from kShaDesc: the descriptors and states of md::sha::Args, the
// digests (20 bytes a message, message order), and for the names of a pack the 20 bytes expected of each and the verdicts
// of md_launch_sha1_names.
constexpr size_t kSha1Bytes = 20;  // a digest
struct Sha1Batch {
  uint64_t *off = nullptr, *len = nullptr;
  uint8_t *type = nullptr;
  uint32_t *index = nullptr;
  md::sha::State *state = nullptr;
  uint8_t *digest = nullptr, *expect = nullptr;
  uint32_t *differs = nullptr;
  std::vector<uint32_t> order;  // the host's copy of index: it is uploaded from here, so it lives as long as the batch
};
// SHA-1 of n messages of the buffer at d_data whose lengths the host knows (host arrays; type null: the bytes as they
// are): orders them longest first, uploads, and launches ceil(longest in blocks / "sha1_launch_blocks") times over a
// shrinking prefix.  Nothing is read back and nothing waited for: off, len, type and *b live until the stream has been.
// Adds messages, blocks and launches to *stats.
int sha1_enqueue(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *off, const uint64_t *len, const uint8_t *type, Sha1Batch *b,
                 md_sha1_stats *stats);
// ---- capi_pack.cpp: what md_pack_index_build (capi_pack_build.cpp) shares with md_pack_open and md_pack_verify ----
// The objects' offsets as the table builder takes them - object i is pack[off[i], end[i]), sorted_off / sorted_obj the
// offsets ascending and whose they are - and the names that are known: n_names names ascending, name k being object
// name_obj[k]'s (null: object k's - the idx's order, every name known).  obj_names (20 bytes an object, or null) and crc
// (or null) go into the table as they are.
struct PackTableIn {
  size_t n = 0, n_names = 0;
  const uint64_t *off = nullptr, *end = nullptr, *sorted_off = nullptr;
  const uint32_t *sorted_obj = nullptr, *name_obj = nullptr, *crc = nullptr;
  const uint8_t *names = nullptr, *obj_names = nullptr;
};
// md_pack_open behind the idx: headers, chains, the deltas' sizes, the last walk.  A REF_DELTA whose base's name is not
// among `names` is MD_PACK_MISSING_BASE and what hangs off it MD_INVALID_PACK_BASE, as ever.  resident: the pack is in
// kHostIn already.  P's checksum and fan-out are the caller's.
int pack_table(md_ctx *ctx, const uint8_t *pack, size_t pack_len, const PackTableIn &in, bool resident, md_pack *P);
// md_pack_verify's rounds with the hash pass, over a pack that is in kHostIn: an object with known[o] is compared with its
// name in the table, one without gets its 20 bytes written to names + 20 o and named[o] = 1 if it decoded
struct PackNameSink {
  const uint8_t *known = nullptr;
  uint8_t *names = nullptr, *named = nullptr;
};
int pack_verify_names(md_ctx *ctx, const md_pack *P, const uint64_t *select, size_t k, int32_t *status, md_pack_result *res,
                      const PackNameSink *sink);
// md_pack_verify's rounds with the link pass (md_pack_graph_build, capi_pack_graph.cpp): behind every round's last apply launch
// the two link kernels run over every object of the round where it stands, into `links` (device arrays, the caller's).  The
// call adds its launches of them and leaves their device time; status[j] is the read's for select[j].
struct PackLinkSink {
  md::pkg::Links links = {};
  uint64_t launches = 0, device_ns = 0;
};
int pack_link_rounds(md_ctx *ctx, const md_pack *P, const uint8_t *pack, const uint64_t *select, size_t k, unsigned flags, int32_t *status,
                     md_pack_result *res, PackLinkSink *links);
// md_pack_read's plan and rounds with the selected objects LEFT ON THE DEVICE (md_pack_diff, capi_pack_diff.cpp): object select[j]
// stands at *d_objs + out_off[j] (out_off: k + 1 entries, back to back as in md_pack_read's dst) until the next call that uses
// kHostOut; nothing but the statuses comes back.  pack == null: the pack is in kHostIn already.  k is not 0.
int pack_read_resident(md_ctx *ctx, const md_pack *P, const uint8_t *pack, const uint64_t *select, size_t k, uint64_t *out_off, int32_t *status,
                       md_pack_result *res, const uint8_t **d_objs);
// ---- capi_pack_graph.cpp: the graph of a pack, as md_pack_diff reads it ----
// The statuses and the CSR's rows on the host, the edges on the device, and of the edges those a history is made of -
// COMMIT_PARENT and TAG_TARGET, with a target - on the host as a CSR of their own.  pack_checksum: of the table it was built from.
struct md_pack_graph {
  int device = 0;
  md_pack_graph_info info = {};
  uint8_t pack_checksum[20] = {0};
  std::vector<int32_t> status;
  std::vector<uint64_t> first, hist_first;
  std::vector<uint32_t> hist_to;
  md::DevBuf d_first, d_to, d_kind;
};
// ---- capi_pack_write.cpp: the delta batch, as md_pack_delta_sizes_* and md_pack_choose_bases (capi_pack_search.cpp) use it too ----
// The pairs as the kernels take them, the distinct bases that have a block, and what their tables need.  A builder calls
// add_base once per distinct base, in the order the tables shall stand in, and pair() for every pair with its base's place.
struct DeltaPlan {
  std::vector<md::pkw::Pair> pairs;
  std::vector<md::pkw::Base> bases;
  md::pkw::TableRoom room;
  md::pkw::TablePlace add_base(uint64_t off, uint64_t len) {
    const md::pkw::TablePlace at = room.add(len);
    if (at.bits) bases.push_back(md::pkw::Base{off, at.table_off, at.first_block, at.bits, 0});
    return at;
  }
  static md::pkw::Pair pair(const md_pack_delta_pair &p, const md::pkw::TablePlace &at) {
    return md::pkw::Pair{p.base_off, p.base_len, p.tgt_off, p.tgt_len, p.out_off, p.out_cap, at.table_off, at.bits, 0};
  }
};
// pairs in the caller's order; the distinct bases are found by sorting the pairs by (base_off, base_len), and stand in that order
void plan_deltas(size_t n, const md_pack_delta_pair *in, DeltaPlan *plan);
// what the second launch over a plan's pairs is: the deltas' bytes, or their lengths alone (md_launch_pks_sizes)
enum class DeltaKind { kWrite, kSizes };
// every pair's length and status on the device.  Both null on the way in: they are carved behind the plan's rows in kPkwDesc
struct DeltaResults {
  uint64_t *out_len = nullptr;
  int32_t *status = nullptr;
};
// On the context's stream: the plan's rows to kPkwDesc, its tables preset in kPkwTables, then pkw_span around the index launch
// (if a base has a block) and the delta or size launch.  d_out: where the deltas go (kSizes: unused).  Nothing is read back.
// Adds the launches to *launches.
int enqueue_delta_plan(md_ctx *ctx, const DeltaPlan &plan, const uint8_t *d_src, DeltaKind kind, uint8_t *d_out, DeltaResults *res,
                       uint64_t *launches);
// md_pack_delta_batch_* and md_pack_delta_sizes_* behind their null checks.  host: src, out and res are the caller's host
// memory, the call uploads, reads back and waits; else they are device memory and the time stays pending.  kSizes: out_off
// is ignored and there is no out.
int delta_batch(md_ctx *ctx, bool host, DeltaKind kind, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint8_t *out,
                size_t out_bytes, DeltaResults res);
// what md_pack_write and md_pack_choose_bases ask of every row: a type of 1 .. 4, the object inside the source and no longer
// than MD_MAX_STREAM.  `who` begins the error's text.
int check_sources(md_ctx *ctx, const char *who, size_t n, const md_pack_source *objs, size_t src_len);
// ---- capi_long_stream.cpp: both return MD_NOT_HANDLED for what the serial path has to answer ----
int continue_parallel(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                      size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status, md_inf_resume *resume);
int inflate_parallel(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *consumed,
                     size_t *written, uint32_t *checksum);
// The complete blocks of a piece decoded by the whole chip and LEFT ON THE DEVICE (md_inflate_index_build): the piece
// src[0, src_len) starts start_bit bits into src[0], hist[0, hist_len) is the output in front of it, `room` bounds the new
// output.  MD_OK: the new bytes are at *d_out (hist_len bytes of window lie in front of them), *status is MD_OK (the final
// block ended; *used bytes of src) or MD_UNEXPECTED_END_OF_INPUT (src ended inside a block), *resume_bits is the bit
// behind the last complete block, and starts receives every block start the verified chain of pieces went through, in
// order, as (bit from src[0], bytes of new output in front of it).
struct ParStart {
  uint64_t bit, out;
};
int continue_parallel_device(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, const uint8_t *hist, size_t hist_len,
                             uint64_t room, const uint8_t **d_out, int *status, uint64_t *total, uint64_t *used, uint64_t *resume_bits,
                             std::vector<ParStart> *starts);
// Adler-32 of n bytes at d (device) going on from `adler`; CRC-32 of the n bytes at d_base + off (complete value)
int par_adler(md_ctx *ctx, const uint8_t *d, uint64_t n, uint32_t adler, uint32_t *res);
int par_crc(md_ctx *ctx, const uint8_t *d_base, uint64_t off, uint64_t n, uint32_t *res);
#pragma GCC visibility pop
