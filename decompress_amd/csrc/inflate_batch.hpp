// inflate_batch.hpp — what the hand-out kernels of inflate_batch.hip read and write for one row of a launch of
// md_inflate_continue_batch_device (md_inf_batch, stream_inf.cpp).  Shared by the kernels and the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace md {
namespace ib {

enum : uint32_t {
  kRowFinal = 1,    // flags: the decoder's end of input is in this piece
  kRowCanGrow = 2,  // flags: the output room is below MD_MAX_STREAM (running out of it asks for more)
};
enum : uint32_t {
  kKindContinue = 0,  // the piece ends inside a block: [hist, resume_out) is handed out, the next piece starts at resume_bits
  kKindFinish = 1,    // the body ended or failed: [hist, out_len) is handed out
  kKindGrow = 2,      // the output room ran out: nothing is handed out, the piece runs again with more room
};

// the inflate kernel's results of one row, where they lie (device arrays of the launch), and the row's descriptors
struct HandIn {
  const uint64_t *out_off, *out_cap, *out_len, *consumed, *resume_bits, *resume_out;
  const uint32_t *hist, *flags, *checksum, *resume_adler;
  const int32_t *status;
};

// per row, written by the hand-out kernels and read back by the host in one copy
struct HandRow {
  uint64_t pack_off;   // where the handed range lies in the packed blob (16-byte aligned)
  uint64_t len;        // its length
  uint64_t tail_bits;  // continue: the next piece starts this many bits into the row's input; finish: bytes the body used * 8
  uint64_t end;        // output position (window included) where the handed range ends
  uint32_t crc;        // CRC-32 of the handed range (GZIP only, else 0)
  uint32_t sum;        // Adler-32 state at `end`
  int32_t status;      // the inflate kernel's status
  uint32_t kind;       // kKind*
};
static_assert(sizeof(HandRow) == 48, "HandRow is copied to the host as is");

}  // namespace ib
}  // namespace md

// m rows of one inflate launch: scan, then pack (res: m HandRow; pack: room for the padded ranges, see stream_inf.cpp)
extern "C" int md_launch_inf_handout(uint32_t m, md::ib::HandIn in, const uint8_t *out, md::ib::HandRow *res, uint8_t *pack,
                                     int with_crc, hipStream_t stream);
