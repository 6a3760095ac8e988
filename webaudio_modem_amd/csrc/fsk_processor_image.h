// fsk_processor_image.h -- the image format of a processor snapshot (include/fskhip_next.h: "FSKP": a ProcHeader, then n_records
// records as fsk_params.h lays them out), and the one definition of what makes an image valid: fskhip_processor_snapshot_info_get,
// fskhip_processor_restore (fsk_processor_remap_api.hip) and a stand-alone check program (tests/cpp/snapshot_image_check.cpp) all
// walk an image with proc_image_open, on fsk_image.h's frame.  The writer's side is here as well: the header and size of an image
// (proc_image_header, proc_image_bytes: fskhip_processor_snapshot's), a record moved to another payload pitch (proc_record_put)
// and, on those, proc_image_concat -- fskhip_processor_snapshot_concat, and tests/cpp/processor_image_concat_check.cpp.
// Host-only: no HIP.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fsk_image.h"
#include "fsk_params.h"

namespace fsk {

constexpr uint32_t kProcMagic = 0x504B5346u;   // "FSKP"
constexpr uint32_t kProcFormat = 1;

struct ProcHeader {
  uint32_t magic, format;
  uint32_t header_bytes, record_bytes;
  uint32_t n_records;
  uint32_t rx_capacity, payload_capacity;   // a record: kProcRecFixed + payload_capacity + rx_capacity rounded up to 16
  uint32_t zero0;
  uint64_t checksum;                        // snap_sum over the header with this field 0, then the records
  uint64_t zero1;
};
static_assert(sizeof(ProcHeader) == 48 && offsetof(ProcHeader, magic) == 0 && offsetof(ProcHeader, format) == 4 && offsetof(ProcHeader, header_bytes) == 8 &&
              offsetof(ProcHeader, n_records) == 16 && offsetof(ProcHeader, checksum) == 32, "ProcHeader is format 1's");

inline uint32_t proc_record_bytes(uint32_t rx_capacity, uint32_t pay_cap) { return kProcRecFixed + pay_cap + (uint32_t)image_round16(rx_capacity); }

// a validated image: the header (copied) and the records in the caller's bytes
struct ProcSnap {
  ProcHeader h;
  const unsigned char *rec;
};

// 0 and *s filled in, or -1 and the flaw named in msg.  Order: the frame's front, rx_capacity, payload_capacity, record_bytes, the
// size against n_records, the checksum, then record by record.
inline int proc_image_open(const void *buf, size_t size, ProcSnap *s, char *msg, size_t msg_cap) {
  ProcHeader &h = s->h;
  if (const int rc = image_open_front("a processor snapshot", buf, size, kProcMagic, kProcFormat, &h, msg, msg_cap)) return rc;
  if (h.rx_capacity == 0 || h.rx_capacity > (1u << 30)) return image_flaw(msg, msg_cap, "rx_capacity %u in the snapshot", h.rx_capacity);
  if ((h.payload_capacity & 15u) != 0u || h.payload_capacity > (1u << 30))
    return image_flaw(msg, msg_cap, "payload_capacity %u in the snapshot (a multiple of 16)", h.payload_capacity);
  if (h.record_bytes != proc_record_bytes(h.rx_capacity, h.payload_capacity))
    return image_flaw(msg, msg_cap, "record_bytes %u, but rx_capacity %u and payload_capacity %u make records of %u bytes", h.record_bytes, h.rx_capacity,
                      h.payload_capacity, proc_record_bytes(h.rx_capacity, h.payload_capacity));
  if (const int rc = image_open_back("n_records", buf, size, h, h.n_records, &s->rec, msg, msg_cap)) return rc;
  // the words a kernel would index with: inside the ring, inside the record's payload
  for (uint32_t r = 0; r < h.n_records; r++) {
    uint32_t w[8];
    std::memcpy(w, s->rec + (size_t)r * h.record_bytes, sizeof(w));
    if (w[0] >= h.rx_capacity || w[1] >= h.rx_capacity || w[2] > h.rx_capacity)
      return image_flaw(msg, msg_cap, "record %u: ring words (writeIndex %u, readIndex %u, _length %u) outside rx_capacity %u", r, w[0], w[1], w[2], h.rx_capacity);
    if (w[3] > 1u || w[7] > h.payload_capacity || (w[6] != 0u && w[5] >= w[6]))
      return image_flaw(msg, msg_cap, "record %u: modulator words (pending %u, position %u of %u, payload %u bytes of %u) are inconsistent", r, w[3], w[5], w[6], w[7],
                        h.payload_capacity);
  }
  return 0;
}

// ---- the writer's side ----
// the header of an image of n records (checksum still 0: image_seal, or a running snap_sum, fills it in) and the image's size
inline ProcHeader proc_image_header(uint32_t n, uint32_t rx_capacity, uint32_t pay_cap) {
  ProcHeader h = image_header<ProcHeader>(kProcMagic, kProcFormat);
  h.record_bytes = proc_record_bytes(rx_capacity, pay_cap); h.n_records = n; h.rx_capacity = rx_capacity; h.payload_capacity = pay_cap;
  return h;
}
inline size_t proc_image_bytes(uint32_t n, uint32_t rx_capacity, uint32_t pay_cap) { return sizeof(ProcHeader) + (size_t)n * proc_record_bytes(rx_capacity, pay_cap); }

// a canonical record of payload capacity src_pay written at payload capacity dst_pay >= src_pay: words, payload, zeros up to
// dst_pay (canonical form: payload bytes beyond the pending payload are zero), ring
inline void proc_record_put(unsigned char *dst, uint32_t dst_pay, const unsigned char *src, uint32_t src_pay, uint32_t rx_capacity) {
  std::memcpy(dst, src, (size_t)kProcRecFixed + src_pay);
  std::memset(dst + kProcRecFixed + src_pay, 0, dst_pay - src_pay);
  std::memcpy(dst + kProcRecFixed + dst_pay, src + kProcRecFixed + src_pay, (size_t)image_round16(rx_capacity));
}

// what proc_image_concat returns beside 0: the values of FSKHIP_E_INVALID and FSKHIP_E_OVERFLOW (this header names no ABI code)
constexpr int kProcConcatInvalid = -1, kProcConcatOverflow = -7;

// out = the records of bufs[0], then bufs[1], ... under one header, in canonical form: the image one processor holding the same
// streams writes.  payload_capacity is canonical per image -- the longest pending payload among ITS records, rounded up to 16 --
// so parts of one batch differ in it as their payloads do: the result takes the largest and every record is written at that
// pitch.  Every part is opened with proc_image_open; parts must agree in rx_capacity.  *written (may be null) receives the size
// whenever the parts are valid; out null or cap too small: kProcConcatOverflow and nothing written.  out overlaps no part.
inline int proc_image_concat(const void *const *bufs, const size_t *sizes, uint32_t n, void *out, size_t cap, size_t *written, char *msg, size_t msg_cap) {
  if (!bufs || !sizes || n == 0) { image_flaw(msg, msg_cap, "null / no snapshots"); return kProcConcatInvalid; }
  std::vector<ProcSnap> ss(n);
  uint64_t total = 0;
  uint32_t pay_cap = 0;
  for (uint32_t k = 0; k < n; k++) {
    char flaw[400];
    if (proc_image_open(bufs[k], sizes[k], &ss[k], flaw, sizeof(flaw))) { image_flaw(msg, msg_cap, "%s (snapshot %u)", flaw, k); return kProcConcatInvalid; }
    const ProcHeader &g = ss[k].h;
    if (g.rx_capacity != ss[0].h.rx_capacity) {
      image_flaw(msg, msg_cap, "snapshots 0 and %u differ in rx_capacity (%u, %u): not images of what could have been one processor", k, ss[0].h.rx_capacity, g.rx_capacity);
      return kProcConcatInvalid;
    }
    total += g.n_records;
    if (g.payload_capacity > pay_cap) pay_cap = g.payload_capacity;
  }
  if (total > 0xFFFFFFFFull) { image_flaw(msg, msg_cap, "%llu records in all", (unsigned long long)total); return kProcConcatInvalid; }
  const ProcHeader h = proc_image_header((uint32_t)total, ss[0].h.rx_capacity, pay_cap);
  const size_t need = proc_image_bytes(h.n_records, h.rx_capacity, pay_cap);
  if (written) *written = need;
  if (!out || cap < need) {
    image_flaw(msg, msg_cap, "the snapshots take %zu bytes together, the buffer has %zu", need, out ? cap : (size_t)0);
    return kProcConcatOverflow;
  }
  unsigned char *rec = (unsigned char *)out + sizeof(ProcHeader);
  for (uint32_t k = 0; k < n; k++) {
    const ProcHeader &g = ss[k].h;
    if (g.payload_capacity == pay_cap) {   // the same pitch: one copy
      const size_t bytes = (size_t)g.n_records * g.record_bytes;
      if (bytes) std::memcpy(rec, ss[k].rec, bytes);
      rec += bytes;
      continue;
    }
    for (uint32_t r = 0; r < g.n_records; r++, rec += h.record_bytes) proc_record_put(rec, pay_cap, ss[k].rec + (size_t)r * g.record_bytes, g.payload_capacity, h.rx_capacity);
  }
  image_seal(h, out, need);
  return 0;
}

}  // namespace fsk
