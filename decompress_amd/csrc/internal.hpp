// internal.hpp — the boundary between the host code and the kernel files: every extern "C" function that a .hip file
// defines and the host calls, the structs that cross, and the constants both sides size things by.  The defining file
// and every caller include it, so a prototype that drifts from its definition does not compile.  Plain host C++.
// (What the host files share among themselves is in ctx.hpp.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdeflate.h"
#include "pack_diff.hpp"
#include "pack_search.hpp"
#include "pack_write.hpp"

// statuses of the library's own, beside mdeflate.h's MD_* (none of which they equal)
constexpr int MD_PIECE_AWAIT = 1000;  // a stream in pieces: the matcher waits for input the piece does not hold
constexpr int MD_NOT_HANDLED = 1001;  // a special path does not take this input: the caller goes the general way

namespace md {
namespace defl {

#ifndef MD_PGM
#define MD_PGM 4
#endif
constexpr uint32_t kChunk = MD_PGM * 64;  // positions per wavefront of the match kernel (PGM steps of 64, deflate_common.hpp)

// Position-indexed workspace of a batch.  Stream i owns positions [slot[i], slot[i + 1]) of link / flg / m / mq.
struct Front {
  const uint32_t *p_end;   // [n]     positions < p_end[i] are inserted ahead (and have a verdict)
  const uint64_t *slot;    // [n + 1]
  const uint32_t *chunk0;  // [n + 1] first kChunk-position chunk of stream i in the match kernel's grid
  const uint32_t *tail;    // [2 n]   hash head of position len - 3 (De matcher): 4th byte 0 / the byte 32 KiB earlier (H7)
  const uint32_t *flags;   // [1]     bit 0: the batch needs more workspace than the caller's size hint allowed
  uint32_t *link;          // low 16 bits: distance to the previous position with the same hash, 0 = none within
                           // 32767; high 16 bits: a fingerprint of the 3 bytes at the position (fp16)
  uint8_t *flg;            // FL_*
  uint32_t *m, *mq;        // longest_match ahead over the full / quartered chain, valid where flg == FL_MATCH
};

// A stream compressed IN PIECES (the encoder of `Def.encode` while input is still arriving, lib/de.ml:4294-4349,
// lib/zl.ml:523-555): the sequential kernel's state - two LDS structs - is written out when the matcher wants input the
// piece does not hold, and read back when the next piece begins.  Every pointer null: whole streams (the batch path).
//   flags[i]  bit 0: the stream's first piece, bit 1: its last one (the end of the input has been signalled), bit 2: the
//             Adler-32 is the kernel's own, carried in the state (else sum[2i] is the caller's running checksum), bit 3:
//             nothing to do for this stream (it ended in an earlier launch of a batch in slices)
//   state     kPieceState bytes per state slot
//   pos[4i]   w0: position of the first byte the input buffer holds (in_off[i] points at it): the piece brings the
//             32 KiB window (and a margin) along; in_len[i] is the length of the input so far, counted like w0
//   pos[4i+1] rebase: positions are 32-bit, so a long stream's origin moves now and then - w0 and in_len count from the
//             new origin, and this (a multiple of 64 KiB, at most the window base) is what the positions in the state
//             the piece before left have to come down by
//   pos[4i+2] the stream's state slot, pos[4i+3] its command queue's slot (whole streams: queue i)
//   sum[2i]   the checksum of the whole input so far (Adler-32 / CRC-32; for gzip always the caller's), [2i+1] its length
//             mod 2^32 (the trailer of the last piece)
// status[i] = MD_PIECE_AWAIT when the piece ended with the matcher waiting for more input.
struct Piece {
  const uint32_t *flags;
  uint8_t *state;
  const uint64_t *pos;
  const uint32_t *sum;
};
constexpr uint32_t kPieceState = 12288;

// Who drives the encoder (mdeflate.h MD_DRIVER_* are the first three; the rest are the library's own)
enum { DRV_ZL = 0, DRV_HIGHER = 1, DRV_CLI = 2,
       DRV_LZ77 = 3,     // De.Lz77.compress alone: the queue fills are written out as commands (md_de_lz77_compress)
       DRV_ENCODE = 4,   // De.Def.encode alone: the input IS the command list of one last block (md_de_def_encode)
       DRV_SCRIPT = 5,   // De.Def.encode driven step by step: the input is a list of operations (md_de_def_run)
       DRV_NS = 6 };     // De.Def.Ns: only the front kernels know it (deflate_ns.hip has the rest)

// What one launch of the sequential kernel (deflate_kernel.hip) takes: md_launch_deflate's argument, the kernel's too.
struct SeqArgs {
  int format, level, qcap, driver, dynamic, matcher;  // the mode of the whole batch
  uint32_t n;
  // the batch descriptors (device arrays of n entries, the blobs they index)
  const uint8_t *in;
  const uint64_t *in_off, *in_len;
  uint8_t *out;
  const uint64_t *out_off, *out_cap;
  uint64_t *out_len;
  int32_t *status;
  uint32_t *checksum;  // or null
  Front fr;            // the front workspace of this batch, filled by md_launch_deflate_plan + md_launch_deflate_front
  int *queue_ws;       // the command queues: qcap words per queue slot (md_deflate_queue_bytes)
  uint64_t *dbg;       // 32 profile words of stream 0 (md_set_option "profile"), or null
  const uint8_t *gz_hdr;  // MD_FORMAT_GZIP: the header every stream begins with, its length, the streams' CRC-32s
  uint32_t gz_hdr_len;
  const uint32_t *gz_crc;
  uint32_t *hist;         // the partial drivers' second result (histograms / replies), or null
  const uint32_t *order;  // launch order (longest first), or null for index order
  Piece pcs;              // every pointer null: whole streams
  // Each stream's tail (the writer of joined spans, deflate_spans.hip), or null: tail[2i] = h, the bit offset of the
  // header of the stream's closing block (its BFINAL bit), tail[2i + 1] = e, the bit offset behind that block's last bit
  // (behind its end-of-block code; a stored block: its byte-aligned end).  Both count from the first byte the launch
  // wrote of the stream, the frame's header included; in pieces the launch that ends the stream writes them, and h is
  // negative (two's complement) when the header went out with an earlier piece.  Garbage unless status[i] is MD_OK.
  // (Null changes no byte and no result; the two notes the words are made from - one LDS store where a closing block's
  // header is put, one scalar move per packing step - are taken either way: they cost less than asking.)
  uint64_t *tail;
  // Where each stream begins to emit (the writer of primed spans), or null: every stream from position 0.
  // first[i] <= in_len[i].  The front kernels see the whole text as the stream it is; the matcher has walked [0, first[i])
  // inserting every position and emitting nothing, and stands at first[i] with nothing pending and a fresh encoder.  The
  // checksum (and a level-0 copy) covers [first[i], in_len[i]).  In pieces the first piece reads it.  Null changes nothing.
  const uint32_t *first;
};

}  // namespace defl

namespace wv {

// A stream decoded in pieces (md_de_inf_continue_host: the `Flush steps of De.Inf.decode while input is still arriving,
// lib/de.ml:1427-1474): the piece starts start_bit bits into its first byte, the output buffer begins with hist_len
// bytes of what was decoded before (the window), the checksum goes on from adler_in; the kernel says where the last
// block that was complete in this piece ended (bit position, output position, checksum state there) so that the next
// piece can start at that block boundary.  All pointers null: a whole stream, nothing to report (the batch path).
struct Cont {
  const uint32_t *start_bit, *hist_len, *adler_in;
  uint64_t *resume_bits, *resume_out;
  uint32_t *resume_adler, *resume_last;
};

// What one launch of the decoder (inflate_wave.hip) takes: md_launch_inflate_wave's argument, the kernel's too.
struct InfArgs {
  int format;
  uint32_t n;
  // the batch descriptors (device arrays of n entries, the blobs they index)
  const uint8_t *in;
  const uint64_t *in_off, *in_len;
  uint8_t *out;
  const uint64_t *out_off, *out_cap;
  uint64_t *out_len, *consumed;
  int32_t *status;
  uint32_t *checksum;  // or null
  uint64_t *dbg;       // the profile words of stream 0 (md_set_option "profile"), or null
  uint32_t *order;     // n words of device scratch for the launch order (longest first), or null for index order
  int waves;           // wavefronts per stream: 2, or 1 (the one-wavefront form of the kernel: same results)
  Cont cont;           // every pointer null: whole streams
};

}  // namespace wv

// One stream's row of piece_gather_kernel (gz_kernels.hip): its region of the new blob, at new_off, is old_len bytes
// from old_off of the old blob followed by fresh_len bytes from fresh_off of the packed fresh bytes.
struct GatherRow {
  uint64_t old_off, old_len, fresh_off, fresh_len, new_off, reserved;
};
static_assert(sizeof(GatherRow) == 48, "GatherRow is uploaded as is: six u64 words");

namespace gzm {
// input bytes one workgroup of the member scan looks at: it leaves one count per span (gz_members.hip)
constexpr uint32_t kMarkSpanBytes = 16384;
}  // namespace gzm

namespace gzs {
// a file whose members do not state their lengths (gz_spec.hip): a candidate needs this many bytes in front of the end
constexpr uint64_t kCandidateMin = 18;
// rule (c): a span whose body is this share of all bodies (1 / kLongShare) or more is not a stream of the batch.  One
// stream runs at 0.13-0.22 GiB/s, the full batch at about 233 GiB/s of output: a ratio of roughly a thousand.
constexpr uint64_t kLongShare = 1024;
// flag[k] of a span: bit 0 = verified, the bits above it = why the batch left it out
constexpr uint32_t kSpanVerified = 1;
constexpr uint32_t kSpanAdmitted = 0, kSpanImplausible = 1, kSpanLong = 2, kSpanNoRoom = 3;
}  // namespace gzs

namespace spn {
// One stream written as joined spans (deflate_spans.hip).  The stored form of a span of n bytes: stored blocks of at
// most 65 535 bytes, all but the last full (the empty text: one empty block).
constexpr uint64_t kStoredMax = 65535;
constexpr uint64_t stored_blocks(uint64_t n) { return n ? (n + kStoredMax - 1) / kStoredMax : 1; }
constexpr uint64_t stored_size(uint64_t n) { return n + 5 * stored_blocks(n); }
// primed spans: a span's stream begins with at most this much of the text in front of it (De.Lz77's window)
constexpr uint64_t kPrime = 32768;
// what stands around the body: the header's bytes (none, Zl.Def's two, Gz.Def's), and by the format the trailer
struct Frame {
  int format;
  uint32_t hdr_len;
  uint8_t hdr[544];
};
constexpr uint32_t trailer_len(int format) { return format == MD_FORMAT_ZLIB ? 4u : format == MD_FORMAT_GZIP ? 8u : 0u; }
// The spans of a call: device arrays of n entries.  in_off .. tail are the deflate launch's descriptors and results (tail:
// SeqArgs::tail, two words per span), adler its checksums, crc md_launch_crc32's (MD_FORMAT_GZIP, else null).  size[i]: the
// bytes span i takes in the body, off (n + 1 entries): their scan.  err: two words preset to 0 - [0] the largest per-stream
// status (positive) of the encoder that is neither MD_OK nor "no room", [1] the least call-level error (negative): a span's
// own, or MD_E_HIP where a tail does not fit its body; stored: the count of stored spans.
struct Spans {
  uint64_t n, len;
  const uint64_t *in_off, *in_len, *slot_off, *out_len, *tail;
  const int32_t *status;
  const uint32_t *adler, *crc;
  uint64_t *size, *off;
  int32_t *err;
  uint64_t *stored;
};
}  // namespace spn

namespace zip {
// One selected entry of a ZIP archive as the host hands it to zip_kernels.hip: the directory's word on it.  name_pos: its
// name in the blob of names that goes along.
struct Row {
  uint64_t header_off, csize, usize, name_pos;
  uint32_t crc;
  uint16_t name_len, method, flags, reserved;
};
static_assert(sizeof(Row) == 48, "Row is uploaded as is");
// kind[e] of segment_kernel: where an entry's bytes are (and whether they are copied)
constexpr uint8_t kSkip = 0, kStored = 1, kDeflated = 2;
}  // namespace zip

namespace zix {
// The index of a long stream (zindex_kernels.hip).  A round of a read lays its pieces end to end: piece j's compressed
// bytes take in_stride(in_len) of the input blob, its slot - window, then output - slot_stride(out_cap) of the scratch.
// The host copies the compressed bytes to where the plan put them, by the same arithmetic.
constexpr uint64_t kWin = 32768;  // a window (zindex.hpp has the host's kWindow)
constexpr uint64_t in_stride(uint64_t in_len) { return ((in_len + 15) & ~(uint64_t)15) + 16; }
constexpr uint64_t slot_stride(uint64_t out_cap) { return ((out_cap + 63) & ~(uint64_t)63) + 64; }
// what a round's plan leaves for the host (u64 words)
constexpr int kPlanCount = 0, kPlanScratch = 1, kPlanIn = 2, kPlanNext = 3, kPlanWords = 4;
// bytes of a range that one wavefront of the gather copies at a time
constexpr uint64_t kGatherSegment = 16384;
// The tables of a read in device memory.  P points: bit / out (the index's), marked (1 bit per piece: a range touches
// it), round_of (the round a piece was decoded in), verdict (0 = good, else the status its ranges get), place (where its
// new output begins in the slots of that round).
struct Tables {
  uint64_t points, size, body_end;  // body_end: the byte of src behind the DEFLATE body (consumed minus the trailer)
  const uint64_t *bit, *out;
  uint32_t *marked, *round_of;
  int32_t *verdict;
  uint64_t *place;
};
// The descriptors of a round, as md_inflate_continue_batch_device takes them, and piece[j] = which piece stream j is.
struct Round {
  uint64_t *in_off, *in_len, *out_off, *out_cap, *out_len, *consumed, *resume_bits, *resume_out;
  uint32_t *start_bit, *hist_len, *adler_in, *checksum, *resume_adler, *resume_last, *piece;
  int32_t *status;
};
}  // namespace zix

namespace bgr {
// Byte ranges of a blocked GZip file (bgzf_read.hip).  A round of a read packs its members back to back into the input
// blob and gives each an output slot of slot_stride(capacity) bytes; the host plans both, by the index alone.
constexpr uint64_t slot_stride(uint64_t cap) { return ((cap + 63) & ~(uint64_t)63) + 64; }
// bytes of a range that one wavefront of the gather copies at a time
constexpr uint64_t kGatherSegment = 16384;
// The members of a round, in member order: device arrays of `count` entries.
struct Round {
  // the index's word: position and length in the blob, slot and capacity in the slots, the offset of the member's first
  // byte in the file's output (ascending strictly: a member without output is never part of a round)
  const uint64_t *mpos, *mlen, *slot, *cap, *u0;
  // the member's own word: md_launch_gzm_headers' results, the inflate launch's status and consumed bytes of the body
  // (copied aside in front of md_launch_gz_finish, which replaces them), and the status behind md_launch_gz_finish
  const uint64_t *body_len, *isize, *inf_consumed;
  const int32_t *hstatus, *inf_status, *status;
  int32_t *verdict;  // 0 = good, else the status the ranges over this member get
};
}  // namespace bgr

namespace pk {
// git packfiles (pack_kernels.hip).  The objects of a pack in idx order: device arrays of n entries.
constexpr uint32_t kNoBase = 0xffffffffu;
// instruction bytes of a delta that one step of the apply kernel looks at: one per lane
constexpr uint32_t kWindow = 64;
// the table md_pack_open builds.  off / end: where the object lies in the pack (the idx's offsets, sorted on the host);
// sorted_off / sorted_obj: the offsets ascending and whose they are; names: n_names names of 20 bytes each, ascending,
// name k being object name_obj[k]'s (name_obj == null: object k's, the idx's order; md_pack_index_build knows only some of
// the names and has its objects in pack order).  The header kernel leaves type (the object's own: 1-4, 6, 7), hsize (the
// size its header states), zoff (where its zlib stream begins), base (kNoBase: none), status, and the chain's first
// state: jump = base, links = 1 for a delta with a base, jump = itself, links = 0 for everything else.
struct Table {
  uint64_t n, pack_len;
  const uint64_t *off, *end, *sorted_off;
  const uint32_t *sorted_obj;
  const uint8_t *names;
  uint8_t *type;
  uint64_t *hsize, *zoff;
  uint32_t *base, *jump, *links;
  int32_t *status;
  uint64_t n_names;
  const uint32_t *name_obj;
};
// One needed zlib stream of a round: its packed bytes (header included) [off, off + packed) and the idx's CRC-32 of them,
// the size its header states; in_len as the inflate launch got it.
struct Stream {
  uint64_t off, packed, in_len, hsize;
  uint32_t crc, reserved;
};
static_assert(sizeof(Stream) == 40, "Stream is uploaded as is");
// One delta of a level of a round.  All offsets count from the start of the round's buffer (the output, then the scratch):
// the payload, the base's bytes, where the result goes.  self / base_slot: the delta's and its base's stream of the round,
// whose statuses it reads and (self) writes.
struct Delta {
  uint64_t pay_off, pay_len, base_off, base_size, out_off, out_size;
  uint32_t self, base_slot;
};
static_assert(sizeof(Delta) == 56, "Delta is uploaded as is");
// a selected object that was selected before: len bytes from src_off to dst_off of the output
struct Repeat {
  uint64_t src_off, dst_off, len;
};
}  // namespace pk

namespace pkw {
// Making deltas (pack_write_kernels.hip; the definition is mdeflate.h's, its constants pack_write.hpp's).  A base is indexed
// by its blocks of kBlock bytes: the hash of a block's four little-endian words, x = (x + w) * kHashMul from 0, picks by its
// top `bits` bits (table_bits) a slot of the base's table of 2^bits words; a slot holds the lowest block index that maps
// to it, kEmpty where none does.
// One distinct base of a call: src[off, off + 16 blocks), its table at tables + table_off (in words), first_block = the
// blocks of the bases in front of it (the index kernel finds a thread's base by it).  Only bases with a block are listed.
struct Base {
  uint64_t off, table_off, first_block;
  uint32_t bits, reserved;
};
static_assert(sizeof(Base) == 32, "Base is uploaded as is");
// One pair: base and target in src, the delta's place in dst, the base's table (bits == 0: the base has no block, no table)
struct Pair {
  uint64_t base_off, base_len, tgt_off, tgt_len, out_off, out_cap, table_off;
  uint32_t bits, reserved;
};
static_assert(sizeof(Pair) == 64, "Pair is uploaded as is");
}  // namespace pkw

namespace pks {
// Choosing bases (pack_search_kernels.hip; the sketch's definition is mdeflate.h's, its constants pack_search.hpp's).
// One segment of an object: the positions [0, npos) from src + off, npos at most kSegPositions; obj: whose features it folds into
struct Seg {
  uint64_t off;
  uint32_t npos, obj;
};
static_assert(sizeof(Seg) == 16, "Seg is uploaded as is");
}  // namespace pks

namespace pkg {
// The object graph of a pack (pack_graph_kernels.hip; the rules are mdeflate.h's, the parse functions pack_graph.hpp's).
// What the link kernels look names up in and where their edges go.  names / fan / type: the idx's names (n of 20 bytes,
// ascending: name k is object k's), its fan-out (fan[b] = the names whose first byte is at most b) and every object's type
// (its root's; 0: not known).  Object o's edges go to to / kind from slot_off[o] on - a slot holds pack_graph.hpp's
// edge_bound of them -, their number to deg[o]; bad[o] = 1: its links cannot be read (deg[o] is 0 then).
struct Links {
  const uint8_t *names;
  const uint32_t *fan;
  const uint8_t *type;
  uint64_t n;
  const uint64_t *slot_off;
  uint32_t *to;
  uint8_t *kind;
  uint32_t *deg;
  uint8_t *bad;
};
// The streams of a round of a read that one of the two kernels looks at, q = slot[0 .. count): object obj[q] of type
// type[q] stands at buf + off[q], size[q] bytes, where the round's last apply launch left it with status[q]
struct Round {
  uint32_t count;
  const uint32_t *slot, *obj;
  const uint64_t *off, *size;
  const uint8_t *type;
  const int32_t *status;
};
// bytes of a tree that one step of the tree kernel looks at: an aligned dword a lane
constexpr uint32_t kTreeWindow = 256;
// One walk over the graph: first / to are the compacted edges (first: n + 1), mark one word an object (0 or 1), next / next_len
// the frontier that a step appends to
struct Reach {
  const uint64_t *first;
  const uint32_t *to;
  uint32_t *mark;
  uint32_t *next, *next_len;
};
}  // namespace pkg

namespace pkd {
// Trees diffed on the device (pack_diff_kernels.hip; the rules are mdeflate.h's, the functions pack_diff.hpp's).  One level of
// md_pack_diff: its distinct trees stand in the read's buffer, tree t at buf + off[t], size[t] bytes, decoded with status[t],
// object obj[t] of the graph.  The table kernel writes tree t's entries as rows from rows + row_off[t] on (a slot holds
// size / 24 of them), their number to cnt[t], and ok[t] = 1: it decoded, every entry is read and the keys ascend strictly.
using Row = pd::Entry;
struct Trees {
  uint32_t count;
  const uint64_t *off, *size, *row_off;
  const int32_t *status;
  const uint32_t *obj;
  Row *rows;
  uint32_t *cnt;
  uint8_t *ok;
};
// The level's pairs: a[q] / b[q] are trees of the level (indices into Trees) or pd::kNone, the empty tree; id[q] and parent[q] go
// into the records as they are.  first / to: the graph's resident edges - tree o's entry e names object to[first[o] + e].
// The count form leaves nrec[q] and nbytes[q] (records, bytes of their names); the write form stores pair q's records from
// out + rec_first[q] on and their names from names + name_first[q] on (the scans of the counts), a record's name_off being
// name_base + its place in names.  A pair with a side that is not ok has no records.
struct Pairs {
  uint32_t count;
  const uint32_t *a, *b, *id, *parent;
  const uint64_t *first;
  const uint32_t *to;
  uint32_t *nrec;
  uint64_t *nbytes;
  const uint64_t *rec_first, *name_first;
  md_tree_change *out;
  uint8_t *names;
  uint64_t name_base;
};
}  // namespace pkd

namespace sha {
// SHA-1 of many messages, one a lane (sha1_kernels.hip).  Message m is data[off[m], off[m] + len[m]) with the header of
// a git object of type[m] in front (1 commit, 2 tree, 3 blob, 4 tag; 0, or type == null: the bytes as they are), len[m] at
// most MD_MAX_STREAM.  Its state between two launches: h[5] and the blocks of 64 bytes done.
struct State {
  uint32_t h[5], done;
};
// md_set_option "sha1_launch_blocks": its range, and the default (DESIGN 4j has the launch time measured for it)
constexpr uint32_t kLaunchBlocksMax = 1u << 24, kLaunchBlocksDefault = 4096;
static_assert(sizeof(State) == 24, "State is six words");
// What one launch takes: md_launch_sha1's argument, the kernel's too.  Lane i of the launch has message index[i] (index ==
// null: message i) and advances it by at most `blocks` blocks; fresh != 0: the first launch of the batch, the states are
// the kernel's to begin.  The launch that ends message m leaves its 20 bytes at digest + 20 m.
struct Args {
  uint32_t count, blocks, fresh;
  const uint8_t *data;
  const uint64_t *off, *len;
  const uint8_t *type;
  const uint32_t *index;
  State *state;
  uint8_t *digest;
};
}  // namespace sha
}  // namespace md

extern "C" {

// ---- inflate_wave.hip ----
int md_launch_inflate_wave(const md::wv::InfArgs *args, hipStream_t stream);
int md_launch_stream_order(uint32_t n, const uint64_t *in_len, uint32_t *order, hipStream_t stream);
// the size query (md_inflate_sizes_batch_device): the count kernel, `order` as above; dbg = null, or three u64 counters the
// streams add to (rounds, passes, rounds that needed the checking walk)
int md_launch_inflate_count(int format, uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint64_t *out_len,
                            uint64_t *consumed, int32_t *status, uint64_t *dbg, uint32_t *order, hipStream_t stream);
// GZIP behind it: body_off / hstatus as md_launch_gz_header leaves them; trailer present, ISIZE, consumed
int md_launch_sizes_gz_finish(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint64_t *body_off,
                              const int32_t *hstatus, uint64_t *out_len, uint64_t *consumed, int32_t *status, hipStream_t stream);
// out_cap = out_len, out_off = the exclusive sum of the caps rounded up to align (a power of two), *total = the whole
int md_launch_inflate_plan(uint64_t n, const uint64_t *out_len, uint64_t align, uint64_t *out_off, uint64_t *out_cap, uint64_t *total,
                           hipStream_t stream);
int md_i_debug_inflate_lds_pad(uint32_t bytes);
int md_i_debug_known_bounds(int mode, uint32_t nstreams);

// ---- inflate_chunked.hip ----
int md_launch_find_blocks(const uint8_t *body, uint64_t nbytes, uint64_t K, uint32_t nchunks_behind_first, uint64_t *cand,
                          hipStream_t stream);
int md_launch_fill_windows(uint32_t n, uint8_t *out, const uint64_t *out_off, const uint8_t *variant, hipStream_t stream);
int md_launch_window_chain(uint32_t npieces, const uint8_t *dst, const uint8_t *scratch, const uint64_t *offa, const uint64_t *offb,
                           const uint64_t *u, uint8_t *wins, uint32_t *flag, hipStream_t stream);
size_t md_windows_work_bytes(uint32_t npieces, uint32_t group);
int md_launch_windows_parallel(uint32_t npieces, uint32_t group, const uint8_t *dst, uint64_t u0, const uint8_t *scratch,
                               const uint64_t *offa, const uint64_t *offb, const uint64_t *u, const uint64_t *pos, uint8_t *wins,
                               uint32_t *work, uint32_t *flag, hipStream_t stream);
int md_launch_resolve(uint32_t npieces, uint8_t *dst, const uint8_t *scratch, const uint64_t *offa, const uint64_t *offb,
                      const uint64_t *u, const uint64_t *pos, const uint8_t *wins, uint32_t *flag, hipStream_t stream);
int md_launch_adler_segments(const uint8_t *data, uint64_t n, uint32_t seg, uint32_t *sums, hipStream_t stream);

// ---- deflate_front.hip: the front workspace (struct Front) and the kernels that fill it ----
size_t md_front_small_bytes(uint32_t n);
size_t md_front_big_bytes(uint64_t positions);
void md_front_carve(void *small_ws, void *big_ws, uint32_t n, uint64_t positions, md::defl::Front *f);
int md_launch_deflate_plan(uint32_t n, const uint64_t *in_len, int driver, int matcher, int level, uint64_t cap_positions,
                           uint32_t cap_chunks, const md::defl::Front *f, hipStream_t stream);
int md_launch_deflate_match(uint32_t n, uint32_t nchunks_max, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                            uint32_t max_chain, uint32_t nice, const md::defl::Front *f, uint32_t match_skip, hipStream_t stream);
int md_launch_deflate_front(uint32_t n, uint32_t nchunks_max, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                            int matcher, uint32_t max_chain, uint32_t nice, const md::defl::Front *f, const uint32_t *order,
                            uint32_t match_skip, hipStream_t stream);
// streams that begin to emit at first[i] (SeqArgs::first): no verdicts for the chunks wholly below it
int md_launch_deflate_front_first(uint32_t n, uint32_t nchunks_max, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                                  int matcher, uint32_t max_chain, uint32_t nice, const md::defl::Front *f, const uint32_t *order,
                                  const uint32_t *first, hipStream_t stream);
int md_launch_link_ns(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const md::defl::Front *f,
                      hipStream_t stream);

// ---- deflate_chunked.hip ----
int md_launch_link_chunked(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t p_end, uint32_t seg,
                           uint32_t cus, const md::defl::Front *f, hipStream_t stream);

// ---- deflate_kernel.hip ----
size_t md_deflate_queue_bytes(uint32_t n, int qcap);
void md_deflate_level_params(int driver, int matcher, int level, uint32_t *max_chain, uint32_t *nice);
int md_launch_deflate(const md::defl::SeqArgs *args, hipStream_t stream);

// ---- deflate_ns.hip ----
int md_launch_def_ns(int format, int level, uint32_t n, uint32_t nchunks_max, const uint8_t *in, const uint64_t *in_off,
                     const uint64_t *in_len, uint8_t *out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                     int32_t *status, uint32_t *checksum, const md::defl::Front *f, hipStream_t stream);

// ---- gz_kernels.hip ----
int md_launch_gz_header(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint64_t *body_off,
                        uint64_t *body_len, int32_t *hstatus, hipStream_t stream);
int md_launch_crc32(uint32_t n, const uint8_t *data, const uint64_t *off, const uint64_t *len, uint32_t *crc_out, hipStream_t stream);
int md_launch_gz_finish(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint64_t *body_off,
                        const int32_t *hstatus, const uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint64_t *consumed,
                        int32_t *status, uint32_t *checksum, hipStream_t stream);
int md_launch_piece_gather(uint32_t n, const uint8_t *old_blob, const uint8_t *fresh, uint8_t *new_blob, const md::GatherRow *d,
                           hipStream_t stream);

// ---- gz_members.hip: a GZip file of many members (md_gz_members_*, md_bgzf_compress) ----
// the scan for members that carry a BC size field: bits = 1 bit per input byte, cnt = one word per kMarkSpanBytes
int md_launch_gzm_mark(const uint8_t *src, uint64_t len, uint32_t *bits, uint32_t *cnt, uint64_t *last_nz, hipStream_t stream);
// out[i] = in[0] + ... + in[i - 1], out[n] = the total
int md_launch_gzm_scan32(const uint32_t *in, uint64_t n, uint64_t *out, hipStream_t stream);
int md_launch_gzm_scan64(const uint64_t *in, uint64_t n, uint64_t *out, hipStream_t stream);
int md_launch_gzm_compact(const uint8_t *src, uint64_t len, const uint32_t *bits, const uint64_t *base, uint64_t *cpos, uint64_t *cnext,
                          hipStream_t stream);
// C candidates; jump_a / jump_b / reach: C + 2 words each.  reach[i] = candidate i is a member of the file, reach[C] = the
// chain from offset 0 ends at the end of the buffer (or at NUL bytes that reach it)
int md_launch_gzm_chain(uint64_t C, const uint64_t *cpos, const uint64_t *cnext, const uint64_t *last_nz, uint32_t *jump_a,
                        uint32_t *jump_b, uint32_t *reach, hipStream_t stream);
int md_launch_gzm_select(uint64_t C, const uint32_t *reach, const uint64_t *ridx, const uint64_t *cpos, const uint64_t *cnext,
                         uint64_t *mpos, uint64_t *mlen, hipStream_t stream);
// body_off / body_len / hstatus as md_launch_gz_header leaves them, for RFC headers; isize from the members' trailers
int md_launch_gzm_headers(uint64_t M, const uint8_t *src, const uint64_t *mpos, const uint64_t *mlen, uint64_t *body_off,
                          uint64_t *body_len, uint64_t *isize, int32_t *hstatus, hipStream_t stream);
// *first (preset to M) = the first member whose status is not MD_OK
int md_launch_gzm_verdict(uint64_t M, const uint64_t *mlen, const uint64_t *consumed, int32_t *status, uint64_t *first, hipStream_t stream);
int md_launch_bgzf_plan(uint64_t nb, uint64_t len, uint64_t block, uint64_t stride, uint64_t *in_off, uint64_t *in_len, uint64_t *out_off,
                        uint64_t *out_cap, hipStream_t stream);
int md_launch_bgzf_sizes(uint64_t nb, const uint64_t *in_len, const uint64_t *out_len, const int32_t *status, uint64_t *msize, int32_t *err,
                         hipStream_t stream);
// moff: nb + 1 member offsets in dst (the scan of msize); the EOF marker goes to moff[nb]
int md_launch_bgzf_pack(uint64_t nb, const uint8_t *src, const uint64_t *in_off, const uint64_t *in_len, const uint8_t *slots,
                        const uint64_t *slot_off, const uint64_t *out_len, const int32_t *status, const uint64_t *moff, const uint32_t *crc,
                        uint8_t *dst, hipStream_t stream);

// ---- deflate_spans.hip: one stream as joined spans (md_deflate_spans_*) ----
// span i = text [i * span, + span) -> stream i of the deflate launch, its slot stored_size(in_len[i]) bytes at i * stride.
// first != null (primed spans): the deflate launch's stream is x_off / x_len - the span and the w = min(i * span, kPrime)
// bytes in front of it - and first[i] = w (SeqArgs::first); in_off / in_len stay the span's own
int md_launch_spans_plan(uint64_t n, uint64_t len, uint64_t span, uint64_t stride, uint64_t *in_off, uint64_t *in_len, uint64_t *out_off,
                         uint64_t *out_cap, uint64_t *x_off, uint64_t *x_len, uint32_t *first, hipStream_t stream);
// adler[i] = the Adler-32 of span i, from the text, for every span whose status is "no room" (the others' are left alone)
int md_launch_spans_adler(const md::spn::Spans *s, const uint8_t *src, uint32_t *adler, hipStream_t stream);
// size[i], err, stored; the scan of size into off is md_launch_gzm_scan64
int md_launch_spans_sizes(const md::spn::Spans *s, hipStream_t stream);
// The whole stream into dst (header, the spans at off[i], trailer) if it fits dst_cap, else nothing.  *written: its length
// (what it needs); *status: MD_OK, MD_UNEXPECTED_END_OF_OUTPUT, or what err says; *checksum: Adler-32 (GZIP: CRC-32) of the text
int md_launch_spans_join(const md::spn::Frame *f, const md::spn::Spans *s, const uint8_t *src, const uint8_t *slots, uint8_t *dst,
                         uint64_t dst_cap, uint64_t *written, int32_t *status, uint32_t *checksum, hipStream_t stream);

// ---- gz_spec.hip: the members of a file without size fields, by speculation (md_gz_members_uncompress) ----
// bits / cnt as md_launch_gzm_mark's; the counts go through md_launch_gzm_scan32
int md_launch_gzs_mark(const uint8_t *src, uint64_t len, uint32_t *bits, uint32_t *cnt, hipStream_t stream);
int md_launch_gzs_compact(uint64_t len, const uint32_t *bits, const uint64_t *base, uint64_t *cpos, hipStream_t stream);
// mlen[k] = cpos[k + 1] - cpos[k], the last span ends at len; md_launch_gzm_headers takes (cpos, mlen) from here
int md_launch_gzs_spans(uint64_t C, const uint64_t *cpos, uint64_t len, uint64_t *mlen, hipStream_t stream);
// *sum_body = the sum of body_len[]; long_min = bytes of body from which rule (c) applies.  pass[k] = guess[k] or 0
int md_launch_gzs_classify(uint64_t C, const int32_t *hstatus, const uint64_t *body_len, const uint64_t *guess, const uint64_t *sum_body,
                           uint64_t long_min, uint64_t *pass, uint8_t *flag, hipStream_t stream);
// out_off = the scan of pass[] (C + 1); leaves in_len (dec_len) / out_off / out_cap of the inflate launch
int md_launch_gzs_room(uint64_t C, const uint64_t *body_len, const uint64_t *pass, uint64_t dst_cap, uint64_t *out_off, uint64_t *dec_len,
                       uint64_t *out_cap, uint8_t *flag, hipStream_t stream);
// behind md_launch_gz_finish
int md_launch_gzs_verify(uint64_t C, const uint64_t *mlen, const int32_t *hstatus, const int32_t *status, const uint64_t *consumed,
                         const uint64_t *out_len, const uint64_t *pass, uint8_t *flag, hipStream_t stream);

// ---- zip_kernels.hip: ZIP archives (md_zip_uncompress, md_zip_compress) ----
// src holds bytes [base, limit) of the archive; in_off / body_off count from base.  kind: md::zip::kSkip / kStored / kDeflated
int md_launch_zip_local(uint64_t k, const md::zip::Row *rows, const uint8_t *src, uint64_t base, uint64_t limit, const uint8_t *names,
                        uint64_t *in_off, uint64_t *in_len, uint64_t *out_cap, uint64_t *body_off, int32_t *hstatus, uint8_t *kind,
                        hipStream_t stream);
// segment s belongs to entry seg_entry[s] and begins (s - first[entry]) * seg bytes into its len[entry] bytes; out may be
// null when every kind is kStored (checksums alone)
int md_launch_zip_segments(uint64_t nseg, uint64_t seg, const uint32_t *seg_entry, const uint64_t *first, const uint64_t *len,
                           const uint8_t *kind, const uint8_t *src, const uint64_t *src_off, uint8_t *out, const uint64_t *out_off,
                           uint32_t *crc, hipStream_t stream);
// status: the inflate launch's on entry, the entries' final ones on return; *failed (preset to 0) counts those not MD_OK
int md_launch_zip_verdict(uint64_t k, const md::zip::Row *rows, const uint64_t *first, uint64_t seg, const uint32_t *crc,
                          const int32_t *hstatus, const uint64_t *out_len, const uint64_t *consumed, int32_t *status, uint64_t *failed,
                          hipStream_t stream);
// the writer.  rec: four words a file (CRC-32, body size, method, offset of the local header); lsize[i] = bytes of local
// header and body; *err (preset to 0) = a status of the encoder that is neither MD_OK nor "no room"
int md_launch_zip_sizes(uint64_t n, int level, const uint64_t *in_len, const uint32_t *name_len, const uint64_t *out_len,
                        const int32_t *status, const uint64_t *first, uint64_t seg, const uint32_t *crc, uint64_t *lsize, uint32_t *rec,
                        int32_t *err, hipStream_t stream);
// loff: n + 1 (the scan of lsize); longest: the longest file, it sizes the grid; dos[i] = time | date << 16
int md_launch_zip_pack(uint64_t n, uint64_t longest, const uint8_t *src, const uint64_t *in_off, const uint64_t *in_len,
                       const uint8_t *slots, const uint64_t *slot_off, const uint8_t *names, const uint64_t *name_pos,
                       const uint32_t *name_len, const uint32_t *dos, const uint64_t *loff, uint32_t *rec, uint8_t *dst, hipStream_t stream);

// ---- zindex_kernels.hip: the index of a long stream (md_inflate_index_build, md_inflate_index_read) ----
// build: window p = the wlen[p] bytes at out + src_off[p] -> wins + p * 32768
int md_launch_zix_windows_take(uint32_t n, const uint8_t *out, const uint64_t *src_off, const uint32_t *wlen, uint8_t *wins,
                               hipStream_t stream);
// read, one round: pieces from `first` on that a range touches (mark != 0: the ranges are marked first; marked[] zeroed by
// the caller), as many as `budget` bytes of slots hold (the first always); plan[kPlan*] and the descriptors
int md_launch_zix_plan(const md::zix::Tables *t, uint64_t n, const uint64_t *off, const uint64_t *len, int mark, uint64_t first,
                       uint64_t budget, uint32_t round, const md::zix::Round *r, uint64_t *plan, hipStream_t stream);
// window j = wins + j * 32768 (hist_len[j] bytes) -> in front of slot j
int md_launch_zix_windows_put(uint32_t count, const uint8_t *wins, const md::zix::Round *r, uint8_t *slots, hipStream_t stream);
int md_launch_zix_verdict(uint32_t count, const md::zix::Tables *t, const md::zix::Round *r, hipStream_t stream);
// the bytes of this round's good pieces into dst + dst_off[i]; status[i] (preset to 0) = the first failing piece's verdict
int md_launch_zix_gather(const md::zix::Tables *t, uint64_t n, uint64_t longest, const uint64_t *off, const uint64_t *len,
                         uint32_t round, const uint8_t *slots, uint8_t *dst, const uint64_t *dst_off, int32_t *status,
                         hipStream_t stream);

// ---- bgzf_read.hip: byte ranges of a blocked GZip file (md_bgzf_read) ----
// behind md_launch_gz_finish: verdict[j] of every member of the round (blob = the round's packed members)
int md_launch_bgr_verdict(uint32_t count, const uint8_t *blob, const md::bgr::Round *r, hipStream_t stream);
// ranges ids[0 .. nr) are those with bytes in this round; longest = the most bytes one of them has in it.  The bytes of the
// round's good members into dst + dst_off[i]; status[i] (preset to 0) = the first failing member's verdict
int md_launch_bgr_gather(uint32_t count, const md::bgr::Round *r, uint32_t nr, const uint32_t *ids, uint64_t longest, const uint64_t *off,
                         const uint64_t *len, const uint8_t *slots, uint8_t *dst, const uint64_t *dst_off, int32_t *status,
                         hipStream_t stream);

// ---- pack_kernels.hip: git packfiles (md_pack_open, md_pack_read) ----
// one thread per object: the header's type / size varint, the base of a delta, Table's results
int md_launch_pk_headers(const md::pk::Table *t, const uint8_t *pack, hipStream_t stream);
// one round of pointer jumping: jump_out[i] = jump_in[jump_in[i]], links_out[i] = links_in[i] + links_in[jump_in[i]]
int md_launch_pk_chain_step(uint64_t n, const uint32_t *jump_in, const uint32_t *links_in, uint32_t *jump_out, uint32_t *links_out,
                            hipStream_t stream);
// behind the last round: root[i] = jump[i] and depth[i] = links[i], or MD_INVALID_PACK where jump[i] is no root (a cycle)
int md_launch_pk_chain_finish(uint64_t n, const uint32_t *jump, const uint32_t *links, uint32_t *root, uint32_t *depth, int32_t *status,
                              hipStream_t stream);
// behind the inflate launch of a round: every stream's final status (crc: md_launch_crc32's of the packed bytes, or null)
int md_launch_pk_verdict(uint32_t count, const md::pk::Stream *s, const uint64_t *out_len, const uint64_t *consumed, const uint32_t *crc,
                         int32_t *status, hipStream_t stream);
// md_pack_open: the two varints in front of a delta payload's instructions (payload j = buf + pay_off[j], s[j].hsize bytes)
int md_launch_pk_delta_sizes(uint32_t count, const md::pk::Stream *s, const uint8_t *buf, const uint64_t *pay_off, uint64_t *base_size,
                             uint64_t *result_size, int32_t *status, hipStream_t stream);
// one level of a round: one wavefront per delta
int md_launch_pk_apply(uint32_t count, const md::pk::Delta *d, uint8_t *buf, int32_t *status, hipStream_t stream);
int md_launch_pk_repeats(uint32_t count, const md::pk::Repeat *r, uint8_t *buf, hipStream_t stream);

// ---- pack_write_kernels.hip: making deltas (md_pack_delta_batch_*) ----
// one thread per block of the nbases listed bases (`blocks` in all) into tables preset to all ones
int md_launch_pkw_index(uint32_t nbases, uint64_t blocks, const md::pkw::Base *bases, const uint8_t *src, uint32_t *tables, hipStream_t stream);
// one wavefront per pair: the delta at dst + out_off, out_len and status (MD_OK, or MD_UNEXPECTED_END_OF_OUTPUT with out_len 0)
int md_launch_pkw_delta(uint32_t count, const md::pkw::Pair *pairs, const uint8_t *src, const uint32_t *tables, uint8_t *dst, uint64_t *out_len,
                        int32_t *status, hipStream_t stream);
// md_pack_write: every object's header bytes (head + kHeaderMax i, head_len[i] of them) and stream (slots + slot_off[i], zlen[i]
// bytes) to pack + offset[i]
int md_launch_pkw_assemble(uint32_t n, const uint64_t *offset, const uint8_t *head, const uint8_t *head_len, const uint8_t *slots,
                           const uint64_t *slot_off, const uint64_t *zlen, uint8_t *pack, hipStream_t stream);

// ---- pack_search_kernels.hip: sketches and count-only deltas (md_pack_sketch_*, md_pack_delta_sizes_*, md_pack_choose_bases) ----
// one wavefront per segment: atomicMin into features + kFeatures * obj, preset to all ones
int md_launch_pks_sketch(uint32_t count, const md::pks::Seg *segs, const uint8_t *src, uint32_t *features, hipStream_t stream);
// one wavefront per pair, against tables md_launch_pkw_index filled: out_len and status as md_launch_pkw_delta's, no delta byte
int md_launch_pks_sizes(uint32_t count, const md::pkw::Pair *pairs, const uint8_t *src, const uint32_t *tables, uint64_t *out_len, int32_t *status,
                        hipStream_t stream);

// ---- pack_graph_kernels.hip: the object graph (md_pack_graph_build, md_pack_reachable) ----
// behind a round's last apply launch: one wavefront per tree of r / one thread per commit or tag of r, the objects in buf
int md_launch_pkg_tree_links(const md::pkg::Round *r, const md::pkg::Links *l, const uint8_t *buf, hipStream_t stream);
int md_launch_pkg_object_links(const md::pkg::Round *r, const md::pkg::Links *l, const uint8_t *buf, hipStream_t stream);
// the edges out of their slots, one thread per edge: to[first[o] .. first[o + 1]) = slot_to[slot_off[o] ..) for every object o
// of the n (first: the scan of Links::deg, first[n] = edges)
int md_launch_pkg_gather(uint64_t n, uint64_t edges, const uint64_t *slot_off, const uint64_t *first, const uint32_t *slot_to,
                         const uint8_t *slot_kind, uint32_t *to, uint8_t *kind, hipStream_t stream);
// mark[seed[k]] = 1 for the count seeds of a walk
int md_launch_pkg_seed(uint32_t count, const uint32_t *seed, uint32_t *mark, hipStream_t stream);
// one wavefront per object of the frontier: its targets marked, those marked first that have edges appended to r->next
int md_launch_pkg_reach_step(const md::pkg::Reach *r, const uint32_t *frontier, uint32_t count, hipStream_t stream);
// out[i] = mark[i] and not excluded[i] (null: nothing is), one byte an object; *count += how many
int md_launch_pkg_reach_finish(uint64_t n, const uint32_t *mark, const uint32_t *excluded, uint8_t *out, uint32_t *count, hipStream_t stream);

// ---- pack_diff_kernels.hip: trees diffed (md_pack_diff) ----
// one wavefront per tree of t, the trees in buf: rows, counts and verdicts
int md_launch_pkd_tree_table(const md::pkd::Trees *t, const uint8_t *buf, hipStream_t stream);
// one wavefront per pair of p over the tables of t: write == 0 counts (nrec, nbytes), else the records and names are stored
int md_launch_pkd_tree_diff(const md::pkd::Trees *t, const md::pkd::Pairs *p, const uint8_t *buf, int write, hipStream_t stream);

// ---- pack_build_kernels.hip: the candidates of md_pack_index_build ----
// bits / cnt as md_launch_gzs_mark's (every word of bits is written: no memset), for the positions of [lo, hi] whose two
// bytes pass the decoder's test of a zlib header; pack is 16-byte aligned and hi + 1 < len.  The counts go through
// md_launch_gzm_scan32, the bits through md_launch_gzs_compact
int md_launch_pkb_mark(const uint8_t *pack, uint64_t len, uint64_t lo, uint64_t hi, uint32_t *bits, uint32_t *cnt, hipStream_t stream);
// in_len[k] = min(end - cpos[k], MD_MAX_INFLATE_IN): the size query's input of candidate k
int md_launch_pkb_inputs(uint64_t C, const uint64_t *cpos, uint64_t end, uint64_t *in_len, hipStream_t stream);

// ---- sha1_kernels.hip: SHA-1 of many messages (md_sha1_batch_*, MD_PACK_VERIFY_NAME) ----
int md_launch_sha1(const md::sha::Args *args, hipStream_t stream);
// differs[j] = the 20 bytes at digest + 20 j are not those at expect + 20 j
int md_launch_sha1_names(uint32_t count, const uint8_t *digest, const uint8_t *expect, uint32_t *differs, hipStream_t stream);

// ---- lzo_kernels.hip ----
// resident workgroups of kind 0: the decoder, 1: the compressor, 2: the count kernel
uint32_t md_lzo_slots(int kind, uint32_t cus);
// the size query (md_lzo_sizes_batch_device): out_len 64-bit and exact, status as mdeflate.h states it
int md_launch_lzo_count(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint64_t *out_len, int32_t *status,
                        uint32_t *counter, uint32_t slots, hipStream_t stream);
int md_launch_lzo_uncompress(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint8_t *out,
                             const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status, uint32_t *counter,
                             uint32_t slots, hipStream_t stream);
int md_launch_lzo_compress(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint8_t *out,
                           const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status, uint16_t *ws_dict,
                           uint32_t *counter, uint32_t slots, hipStream_t stream);

}  // extern "C"
