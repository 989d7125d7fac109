// capi.cpp — host side of the C ABI declared in include/mdeflate.h: contexts, options, timing, status strings.  The
// entry points of each area are in capi_inflate / capi_long_stream / capi_deflate / capi_gz_members / capi_zip / capi_zindex / capi_lzo / capi_pack /
// capi_sha1.cpp.
// Plain HIP runtime calls; no torch types anywhere in this library.
#include <string.h>

#include <string>

#include "ctx.hpp"

namespace {
thread_local std::string g_err;  // what md_last_error_string(NULL) reads: the reason fail() has ONE definition

bool is_gfx950(int dev) {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}
}  // namespace

int fail(md_ctx *ctx, int code, const char *what, hipError_t e) {
  std::string m = what;
  if (e != hipSuccess) {
    m += ": ";
    m += hipGetErrorString(e);
  }
  if (ctx) ctx->err = m;
  g_err = m;
  return code;
}

int md_version(void) { return MD_VERSION; }

// contiguous ranges of the stream index balanced by bytes (decompress_amd/shard.py shard_by_bytes is
// the same arithmetic, in doubles): rank r's range ends with the last stream whose middle lies at or before r + 1
// world-ths of the total.
int md_shard_plan(uint64_t n, const uint64_t *lengths, int world, uint64_t *lo, uint64_t *hi) {
  if (world < 1 || !lo || !hi || (n && !lengths)) return MD_E_INVALID_ARGUMENT;
  double total = 0.0;
  for (uint64_t i = 0; i < n; i++) total += (double)lengths[i];
  double acc = 0.0;
  uint64_t at = 0;
  for (int r = 0; r < world; r++) {
    const double target = total * (double)(r + 1) / (double)world;
    uint64_t end = at;
    while (end < n && acc + (double)lengths[end] / 2.0 <= target) {
      acc += (double)lengths[end];
      end++;
    }
    if (r == world - 1) end = n;
    lo[r] = at;
    hi[r] = end;
    at = end;
  }
  return MD_OK;
}

const char *md_status_string(int s) {
  switch (s) {
  case MD_OK: return "Ok";
  case MD_UNEXPECTED_END_OF_INPUT: return "Unexpected end of input";
  case MD_UNEXPECTED_END_OF_OUTPUT: return "Unexpected end of output";
  case MD_INVALID_KIND_OF_BLOCK: return "Invalid kind of block";
  case MD_INVALID_DICTIONARY: return "Invalid dictionary";
  case MD_INVALID_COMPLEMENT_OF_LENGTH: return "Invalid complement of length";
  case MD_INVALID_DISTANCE: return "Invalid distance";
  case MD_INVALID_DISTANCE_CODE: return "Invalid distance code";
  case MD_INVALID_HEADER: return "Invalid Zlib header";
  case MD_INVALID_CHECKSUM: return "Invalid checksum";
  case MD_INVALID_GZIP_HEADER: return "Invalid GZip header";
  case MD_INVALID_GZIP_HEADER_CHECKSUM: return "Invalid GZip header checksum";
  case MD_INVALID_SIZE: return "Invalid input size";
  case MD_QUEUE_FULL: return "Queue.Full";
  case MD_LZO_INVALID_INPUT: return "Invalid input";
  case MD_LZO_NO_DICTIONARY: return "No dictionary at offset 0 available";
  case MD_LZO_OUT_OF_BOUND: return "Input is malformed or output is not large enough";
  case MD_LZO_MALFORMED_INPUT: return "Malformed input";
  case MD_INVALID_ZIP_DIRECTORY: return "Invalid ZIP directory";
  case MD_INVALID_ZIP_HEADER: return "Invalid ZIP local header";
  case MD_ZIP_UNSUPPORTED: return "Unsupported ZIP entry";
  case MD_INVALID_INDEX: return "Invalid index";
  case MD_INVALID_PACK: return "Invalid pack";
  case MD_INVALID_DELTA: return "Invalid delta";
  case MD_INVALID_PACK_BASE: return "Invalid delta base";
  case MD_PACK_MISSING_BASE: return "Missing delta base";
  case MD_PACK_UNSUPPORTED: return "Unsupported pack";
  case MD_E_INVALID_ARGUMENT: return "Invalid argument";
  case MD_E_NO_DEVICE: return "No gfx950 device";
  case MD_E_HIP: return "HIP runtime error";
  case MD_E_OUT_OF_MEMORY: return "Out of device memory";
  default: return "Unknown status";
  }
}

const char *md_last_error_string(const md_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_err.c_str();
}

int md_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int d = 0; d < n; d++)
    if (is_gfx950(d)) ok++;
  return ok;
}

md_ctx *md_create(int device, void *hip_stream) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    fail(nullptr, MD_E_NO_DEVICE, "md_create: no such HIP device");
    return nullptr;
  }
  if (!is_gfx950(device)) {
    fail(nullptr, MD_E_NO_DEVICE, "md_create: device is not gfx950 (kernels are built for MI355X only)");
    return nullptr;
  }
  md_ctx *ctx = new md_ctx();
  ctx->device = device;
  md::DeviceGuard guard(device);
  if (!guard.ok) {
    delete ctx;
    fail(nullptr, MD_E_HIP, "hipSetDevice");
    return nullptr;
  }
  if (hip_stream == MD_STREAM_NULL) {
    ctx->stream = nullptr;  // the device's legacy default stream: ordered with everything else enqueued on it
  } else if (hip_stream) {
    ctx->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      fail(nullptr, MD_E_HIP, "hipStreamCreate");
      return nullptr;
    }
    ctx->own_stream = true;
  }
  for (md::EventSpan *span : {&ctx->timing, &ctx->sha1_span, &ctx->pkw_span})
    for (hipEvent_t &ev : span->ev)
      if (hipEventCreate(&ev) != hipSuccess) {
        md_destroy(ctx);
        fail(nullptr, MD_E_HIP, "hipEventCreate");
        return nullptr;
      }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->cus = cus;
    if (ctx->counters.reserve(ctx, 256, "hipMalloc(counters)") != MD_OK) {
      md_destroy(ctx);
      return nullptr;
    }
  }
  {  // the deflate kernels' per-position workspace takes a sixth of the device at most (48 GiB of 288) unless told otherwise
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) ctx->front_cap_bytes = mem_total / 6;
  }
  return ctx;
}

void md_destroy(md_ctx *ctx) {
  if (!ctx) return;
  md::DeviceGuard guard(ctx->device);
  for (md::EventSpan *span : {&ctx->timing, &ctx->sha1_span, &ctx->pkw_span})
    for (hipEvent_t ev : span->ev)
      if (ev) hipEventDestroy(ev);
  if (ctx->s_in) hipStreamDestroy(ctx->s_in);
  if (ctx->s_out) hipStreamDestroy(ctx->s_out);
  if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;  // (its buffers free themselves, on the context's device)
}

int md_synchronize(md_ctx *ctx) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  MD_ON_DEVICE(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MD_OK;
}

int md_timing_begin(md_ctx *ctx) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  MD_ON_DEVICE(ctx);
  HIP_TRY(ctx, ctx->timing.begin(ctx->stream));
  return MD_OK;
}

int md_timing_end(md_ctx *ctx, float *ms) {
  if (!ctx || !ms) return MD_E_INVALID_ARGUMENT;
  MD_ON_DEVICE(ctx);
  HIP_TRY(ctx, ctx->timing.end(ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(ctx->timing.ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->timing.ev[0], ctx->timing.ev[1]));
  return MD_OK;
}

void *md_host_alloc(md_ctx *ctx, size_t bytes) {
  if (!ctx) return nullptr;
  md::DeviceGuard guard(ctx->device);
  void *p = nullptr;
  if (!guard.ok || hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    fail(ctx, MD_E_OUT_OF_MEMORY, "hipHostMalloc");
    return nullptr;
  }
  return p;
}
void md_host_free(md_ctx *ctx, void *p) {
  (void)ctx;  // (pinned memory is freed whatever the current device is - and a buffer may outlive its context)
  if (p) hipHostFree(p);
}

int md_set_option(md_ctx *ctx, const char *key, int value) {
  if (!ctx || !key) return MD_E_INVALID_ARGUMENT;
  if (!strcmp(key, "profile")) {  // in-kernel phase profile of stream 0 (debug builds of the kernel)
    if (value && !ctx->dbg.p) {
      const int rc = ctx->dbg.reserve(ctx, 32 * 8, "hipMalloc");
      if (rc != MD_OK) return rc;
      if (hipMemset(ctx->dbg.p, 0, 32 * 8) != hipSuccess) return fail(ctx, MD_E_HIP, "hipMemset");
    } else if (!value) {
      ctx->dbg.release();
    }
    return MD_OK;
  }
  if (!strcmp(key, "inflate_waves")) {
    if (value != 1 && value != 2) return fail(ctx, MD_E_INVALID_ARGUMENT, "inflate_waves is 1 or 2");
    ctx->inflate_waves = value;
    return MD_OK;
  }
  if (!strcmp(key, "deflate_workspace_cap_mib")) {  // 0 = no cap (one launch of each kernel per batch whatever it takes)
    if (value < 0) return fail(ctx, MD_E_INVALID_ARGUMENT, "deflate_workspace_cap_mib >= 0");
    ctx->front_cap_bytes = (size_t)value << 20;
    return MD_OK;
  }
  if (!strcmp(key, "encoder_piece_bytes")) {
    if (value < 1) return fail(ctx, MD_E_INVALID_ARGUMENT, "encoder_piece_bytes >= 1");
    ctx->piece_bytes = (size_t)value;
    return MD_OK;
  }
  if (!strcmp(key, "release_workspace")) {  // give the grow-only scratch of this context back (it grows again on demand)
    MD_ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (md::DevBuf &b : ctx->scratch) b.release();
    return MD_OK;
  }
  if (!strcmp(key, "deflate_test_flags")) {
    ctx->test_flags = value;
    return MD_OK;
  }
  if (!strcmp(key, "inflate_parallel_min")) {  // KiB of compressed input from which ONE stream is decoded in pieces by the whole chip; 0 = never
    if (value < 0) return fail(ctx, MD_E_INVALID_ARGUMENT, "inflate_parallel_min >= 0 (KiB)");
    ctx->par_min = (size_t)value << 10;
    return MD_OK;
  }
  if (!strcmp(key, "inflate_parallel_chunk")) {  // KiB of compressed input per piece
    if (value < 4 || value > (1 << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "inflate_parallel_chunk is 4 .. 2^20 (KiB)");
    ctx->par_chunk = (size_t)value << 10;
    return MD_OK;
  }
  if (!strcmp(key, "inflate_parallel_last")) {  // (query, value ignored) pieces of the last stream that went that way | rounds << 24; 0: it did not
    return ctx->par_last_pieces | (ctx->par_last_rounds << 24);
  }
  if (!strcmp(key, "deflate_link_segment_min")) {  // KiB of input from which ONE stream's hash chains are built in segments; 0 = never
    if (value < 0) return fail(ctx, MD_E_INVALID_ARGUMENT, "deflate_link_segment_min >= 0 (KiB)");
    ctx->link_seg_min = (size_t)value << 10;
    return MD_OK;
  }
  if (!strcmp(key, "deflate_link_segment")) {  // KiB of input per segment; 0 = by the stream's length
    if (value < 0 || value > (1 << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "deflate_link_segment is 0 .. 2^20 (KiB)");
    ctx->link_seg = (size_t)value << 10;
    return MD_OK;
  }
  if (!strcmp(key, "deflate_span_kib")) {  // KiB of text per span of md_deflate_spans_* called with span = 0; 0 = the default
    if (value < 0 || value > (int)(MD_MAX_STREAM >> 10)) return fail(ctx, MD_E_INVALID_ARGUMENT, "deflate_span_kib is 0 .. MD_MAX_STREAM / 1024");
    ctx->span_bytes = value ? (size_t)value << 10 : md::kSpanDefault;
    return MD_OK;
  }
  if (!strcmp(key, "deflate_span_prime")) {  // md_deflate_spans_*: 1 = every span's matcher starts from the 32 KiB of text in front of it
    if (value != 0 && value != 1) return fail(ctx, MD_E_INVALID_ARGUMENT, "deflate_span_prime is 0 or 1");
    ctx->span_prime = value != 0;
    return MD_OK;
  }
  if (!strcmp(key, "gz_members_speculate")) {  // md_gz_members_uncompress, a file without size fields: 1 = members found by speculation, one batch
    if (value != 0 && value != 1) return fail(ctx, MD_E_INVALID_ARGUMENT, "gz_members_speculate is 0 or 1");
    ctx->gzm_speculate = value != 0;
    return MD_OK;
  }
  if (!strcmp(key, "zip_crc_segment")) {  // KiB of an entry's output per wavefront of md_zip_*'s copy-and-checksum kernel; 0 = the default
    if (value != 0 && (value < 4 || value > (1 << 20))) return fail(ctx, MD_E_INVALID_ARGUMENT, "zip_crc_segment is 0 or 4 .. 2^20 (KiB)");
    ctx->zip_segment = value ? (size_t)value << 10 : md::kZipSegmentDefault;
    return MD_OK;
  }
  if (!strcmp(key, "index_read_workspace")) {  // MiB of piece scratch per round of md_inflate_index_read; 0 = one piece a round
    if (value < 0 || value > (1 << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "index_read_workspace is 0 .. 2^20 (MiB)");
    ctx->zix_workspace = (size_t)value << 20;
    return MD_OK;
  }
  if (!strcmp(key, "pack_workspace")) {  // MiB of scratch per round of md_pack_open / md_pack_read; 0 = one selected object a round
    if (value < 0 || value > (1 << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "pack_workspace is 0 .. 2^20 (MiB)");
    ctx->pack_workspace = (size_t)value << 20;
    return MD_OK;
  }
  if (!strcmp(key, "sha1_launch_blocks")) {  // blocks of 64 bytes by which one launch of the SHA-1 kernel advances a message
    if (value < 1 || value > (int)md::sha::kLaunchBlocksMax) return fail(ctx, MD_E_INVALID_ARGUMENT, "sha1_launch_blocks is 1 .. 2^24");
    ctx->sha1_launch_blocks = (uint32_t)value;
    return MD_OK;
  }
  if (!strcmp(key, "bgzf_read_workspace")) {  // MiB of packed input and output slots per round of md_bgzf_read; 0 = one member a round
    if (value < 0 || value > (1 << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "bgzf_read_workspace is 0 .. 2^20 (MiB)");
    ctx->bgr_workspace = (size_t)value << 20;
    return MD_OK;
  }
  if (!strcmp(key, "host_pipeline_slices")) {  // md_*_batch_host: slices of streams in flight (1 = no overlap of copies and kernels)
    if (value < 1 || value > 64) return fail(ctx, MD_E_INVALID_ARGUMENT, "host_pipeline_slices is 1 .. 64");
    ctx->host_slices_max = value;
    return MD_OK;
  }
  if (!strcmp(key, "debug_known_bounds")) {  // measurement builds only (-DMD_DEBUG_KNOWN_BOUNDS): mode | streams << 5
    MD_ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (value < 0 || md_i_debug_known_bounds(value & 31, (uint32_t)value >> 5)) return fail(ctx, MD_E_INVALID_ARGUMENT, "debug_known_bounds: not a measurement build");
    return MD_OK;
  }
  if (!strcmp(key, "debug_inflate_lds_pad")) {  // measurement only: unused LDS per stream, i.e. fewer streams per CU
    MD_ON_DEVICE(ctx);
    if (value < 0 || md_i_debug_inflate_lds_pad((uint32_t)value)) return fail(ctx, MD_E_INVALID_ARGUMENT, "debug_inflate_lds_pad");
    return MD_OK;
  }
  return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown option");
}

// copies the 32 profile words of the last v2 launch to host (after synchronising)
int md_get_profile(md_ctx *ctx, uint64_t *out32) {
  if (!ctx || !out32 || !ctx->dbg.p) return MD_E_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out32, ctx->dbg.p, 32 * 8, hipMemcpyDeviceToHost));
  return MD_OK;
}

int md_crc32_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *d_off,
                          const uint64_t *d_len, uint32_t *d_crc) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull || !d_off || !d_len || !d_crc) return fail(ctx, MD_E_INVALID_ARGUMENT, "bad crc32 batch");
  MD_ON_DEVICE(ctx);
  MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_data, d_off, d_len, d_crc, ctx->stream));
  return MD_OK;
}
