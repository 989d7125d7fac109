// host_pipeline.hpp — a batch of host buffers through the device in slices of streams (md_inflate_batch_host,
// md_deflate_batch_host).
#pragma once
#include <vector>

#include "ctx.hpp"

#pragma GCC visibility push(hidden)

// ---- host buffers in, host buffers out (the reference's callers own host bigarrays, lib/de.mli:93-106) ----------------
// The batch goes through the device in SLICES of consecutive streams: the copy-in of slice k + 1 (stream s_in) and the
// copy-out of slice k - 1 (stream s_out) run under the kernels of slice k (the context's stream); events order the three.
// A slice copies the byte range its streams span in the caller's blob (ranges of different slices may overlap or lie in
// any order: a byte copied twice is copied with the same value, and an output range is final when its slice's kernels
// are).  With pinned host buffers (hipHostMalloc / hipHostRegister) the copies are DMA transfers and really overlap;
// pageable buffers go through the runtime's staging and mostly do not.  The device copies of the blobs are the context's,
// grow-only (md_set_option "release_workspace" gives them back).
struct HostSlice {
  size_t i0, i1;
  uint64_t in_lo, in_hi, out_lo, out_hi;
};
// slices of about equal bytes (input + output room), at least min_streams streams each, at most max_slices
inline std::vector<HostSlice> host_slices(size_t n, const uint64_t *in_off, const uint64_t *in_len, const uint64_t *out_off,
                                          const uint64_t *out_cap, size_t min_streams, size_t max_slices, uint64_t in_bytes, uint64_t out_bytes) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) total += in_len[i] + out_cap[i];
  size_t want = (size_t)(total / ((uint64_t)64 << 20));
  if (want > max_slices) want = max_slices;
  if (min_streams && want > n / min_streams) want = n / min_streams;
  if (want < 1) want = 1;
  std::vector<HostSlice> v;
  uint64_t acc = 0, span = 0;
  size_t i0 = 0;
  for (size_t k = 0; k < want; k++) {
    const uint64_t upto = total / want * (k + 1);
    size_t i1 = i0;
    while (i1 < n && (k + 1 == want || acc < upto || i1 - i0 < min_streams)) {  // (never fewer than min_streams, whatever the sizes: ADVICE r5)
      acc += in_len[i1] + out_cap[i1];
      i1++;
    }
    if (i1 == i0) continue;
    HostSlice sl{i0, i1, ~0ull, 0, ~0ull, 0};
    for (size_t i = i0; i < i1; i++) {
      if (in_len[i]) {
        sl.in_lo = in_off[i] < sl.in_lo ? in_off[i] : sl.in_lo;
        sl.in_hi = in_off[i] + in_len[i] > sl.in_hi ? in_off[i] + in_len[i] : sl.in_hi;
      }
      if (out_cap[i]) {
        sl.out_lo = out_off[i] < sl.out_lo ? out_off[i] : sl.out_lo;
        sl.out_hi = out_off[i] + out_cap[i] > sl.out_hi ? out_off[i] + out_cap[i] : sl.out_hi;
      }
    }
    if (sl.in_hi <= sl.in_lo) sl.in_lo = sl.in_hi = 0;
    if (sl.out_hi <= sl.out_lo) sl.out_lo = sl.out_hi = 0;
    span += (sl.in_hi - sl.in_lo) + (sl.out_hi - sl.out_lo);
    v.push_back(sl);
    i0 = i1;
  }
  // a layout whose slices span much more than the blobs hold (streams scattered across the blob): one slice, whole blobs
  // (a batch that is one slice anyway copies the span of its streams like any other slice: the caller's blobs may hold
  // more than this batch - md_inflate_batch_host picks streams out of one)
  if (v.empty() || (v.size() > 1 && span > in_bytes + out_bytes + (in_bytes + out_bytes) / 4)) {
    v.clear();
    v.push_back(HostSlice{0, n, 0, in_bytes, 0, out_bytes});
  }
  return v;
}
struct EventList {
  std::vector<hipEvent_t> ev;
  ~EventList() {
    for (hipEvent_t e : ev) hipEventDestroy(e);
  }
  hipEvent_t make() {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    ev.push_back(e);
    return e;
  }
};

// `launch(i0, count)` enqueues the device entry point for streams [i0, i0 + count) on ctx->stream
template <class Launch>
int host_pipeline(md_ctx *ctx, const std::vector<HostSlice> &sl, const uint8_t *h_in, uint8_t *d_in, uint8_t *h_out, uint8_t *d_out,
                  Launch launch) {
  if (!ctx->s_in && hipStreamCreateWithFlags(&ctx->s_in, hipStreamNonBlocking) != hipSuccess) return fail(ctx, MD_E_HIP, "hipStreamCreate");
  if (!ctx->s_out && hipStreamCreateWithFlags(&ctx->s_out, hipStreamNonBlocking) != hipSuccess) return fail(ctx, MD_E_HIP, "hipStreamCreate");
  EventList evs;
  // From the first enqueue on there is NO early return: an error is recorded, the loop is left, and the three streams are
  // synchronised before the call returns - the copies read and write the caller's h_in / h_out, and the context's device
  // blobs may be grown (freed) by the next call.
  int rc = MD_OK;
  hipError_t herr = hipSuccess;
  const char *hwhat = nullptr;
#define MD_PIPE_TRY(expr)                       \
  if (rc == MD_OK && herr == hipSuccess) {      \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) {                     \
      herr = e_;                                \
      hwhat = #expr;                            \
    }                                           \
  }
  // (whatever the caller queued on the context's stream before this call comes first, also for the copy streams)
  hipEvent_t e0 = evs.make();
  if (!e0) return fail(ctx, MD_E_HIP, "hipEventCreate");  // (nothing enqueued yet)
  MD_PIPE_TRY(hipEventRecord(e0, ctx->stream));
  MD_PIPE_TRY(hipStreamWaitEvent(ctx->s_in, e0, 0));
  for (size_t k = 0; k < sl.size() && rc == MD_OK && herr == hipSuccess; k++) {
    hipEvent_t e_in = evs.make(), e_k = evs.make();
    if (!e_in || !e_k) {
      herr = hipErrorOutOfMemory;
      hwhat = "hipEventCreate";
      break;
    }
    if (sl[k].in_hi > sl[k].in_lo)
      MD_PIPE_TRY(hipMemcpyAsync(d_in + sl[k].in_lo, h_in + sl[k].in_lo, sl[k].in_hi - sl[k].in_lo, hipMemcpyHostToDevice, ctx->s_in));
    MD_PIPE_TRY(hipEventRecord(e_in, ctx->s_in));
    MD_PIPE_TRY(hipStreamWaitEvent(ctx->stream, e_in, 0));
    if (herr != hipSuccess) break;
    rc = launch(sl[k].i0, sl[k].i1 - sl[k].i0);
    if (rc != MD_OK) break;
    MD_PIPE_TRY(hipEventRecord(e_k, ctx->stream));
    MD_PIPE_TRY(hipStreamWaitEvent(ctx->s_out, e_k, 0));
    if (sl[k].out_hi > sl[k].out_lo)
      MD_PIPE_TRY(hipMemcpyAsync(h_out + sl[k].out_lo, d_out + sl[k].out_lo, sl[k].out_hi - sl[k].out_lo, hipMemcpyDeviceToHost, ctx->s_out));
  }
#undef MD_PIPE_TRY
  // everything in flight ends before the call returns (also after an error: the buffers are the caller's)
  hipError_t a = hipStreamSynchronize(ctx->s_in), b2 = hipStreamSynchronize(ctx->stream), c = hipStreamSynchronize(ctx->s_out);
  if (rc != MD_OK) return rc;
  if (herr != hipSuccess) return fail(ctx, MD_E_HIP, hwhat, herr);
  if (a != hipSuccess || b2 != hipSuccess || c != hipSuccess) return fail(ctx, MD_E_HIP, "host pipeline", a != hipSuccess ? a : b2 != hipSuccess ? b2 : c);
  return MD_OK;
}
#pragma GCC visibility pop
