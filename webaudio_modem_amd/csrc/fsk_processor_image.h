// fsk_processor_image.h -- the image format of a processor snapshot (include/fskhip_next.h: "FSKP": a ProcHeader, then n_records
// records as fsk_params.h lays them out), and the one definition of what makes an image valid: fskhip_processor_snapshot_info_get,
// fskhip_processor_restore (fsk_processor_remap_api.hip) and a stand-alone check program (tests/cpp/snapshot_image_check.cpp) all
// walk an image with proc_image_open, on fsk_image.h's frame.  Host-only: no HIP.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

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

}  // namespace fsk
