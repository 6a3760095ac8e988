// fsk_snapshot_image.h -- the image format of a stream snapshot (include/fskhip.h: "FSKS": a SnapHeader, then n_streams records of
// a SnapRecordHost and the device's sections), and the one definition of what makes an image valid: fskhip_snapshot_info_get,
// _stream_config, _concat, fskhip_restore_streams (fsk_snapshot_api.hip) and a stand-alone check program
// (tests/cpp/snapshot_image_check.cpp) all walk an image with snap_image_open, on fsk_image.h's frame.  Host-only.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/fskhip.h"
#include "fsk_image.h"
#include "fsk_params.h"

namespace fsk {

constexpr uint32_t kSnapMagic = 0x534B5346u;   // "FSKS"
constexpr uint32_t kSnapFormat = 1;

// fskhip_config without the padding its int32 / double mix leaves: every byte of a snapshot is defined
struct SnapConfig {
  double sampleRate, baudRate, markFrequency, spaceFrequency, syncThreshold, preFilterBandwidth;
  int32_t preamblePattern[FSKHIP_MAX_PATTERN_BYTES], sfdPattern[FSKHIP_MAX_PATTERN_BYTES];
  int32_t preambleLen, sfdLen, startBits, stopBits, parity, agcEnabled, adaptiveThreshold, zero;
};
static_assert(sizeof(SnapConfig) == 6 * 8 + (2 * FSKHIP_MAX_PATTERN_BYTES + 8) * 4, "SnapConfig has padding");

struct SnapHeader {
  uint32_t magic, format;
  uint32_t rf_count, if_count;    // the state-layout stamp: the field counts and ...
  uint64_t fields_hash;           // ... FNV-1a of the field names in fsk_params.h order (and the spans the fp32 reset words count in)
  uint64_t checksum;              // snap_sum over the header with this field 0, then the records
  uint32_t header_bytes, record_bytes;
  uint32_t n_streams;
  int32_t precision;
  uint32_t per_stream_configs;    // 0: every record runs under cfg0
  uint32_t d, amp_cap, wide, frac, n_bits, ring_cap;    // the geometry fskhip_remap_streams compares
  uint32_t ds_parity, ds_uniform, gen_odd, quality;     // engine-level values a destination takes over
  uint32_t grid_poly_phase, grid_amp_pos;               // the ring grid: source row 0's positions (every row's, in lock step)
  uint32_t frame_valid;           // fp32, one shared configuration, at least one stream: frame_phase is the engine's
  uint32_t zero[2];
  uint64_t frame_phase;           // the free-running I/Q frame: NCO phase minus frame offset of source row 0 (64-bit turns)
  uint64_t calls, total_samples, pushes;
  SnapConfig cfg0;
};
static_assert(sizeof(SnapHeader) == 352 && offsetof(SnapHeader, magic) == 0 && offsetof(SnapHeader, format) == 4 && offsetof(SnapHeader, checksum) == 24 &&
              offsetof(SnapHeader, header_bytes) == 32 && offsetof(SnapHeader, n_streams) == 40, "SnapHeader is format 1's");

// the host part of a record (kSnapHostWords words): what of a stream lives on the host
struct SnapRecordHost {
  double markFrequency, spaceFrequency, preFilterBandwidth;
  uint32_t adaptiveThreshold, zero;
  uint64_t base_calls, base_samples;
};
static_assert(sizeof(SnapRecordHost) == kSnapHostWords * 4, "SnapRecordHost has padding");

inline uint64_t fields_hash() {
  static const char names[] =
#define X(n) #n ","
      FSK_REAL_FIELDS(X) FSK_REAL_FIELDS_PIPE(X) FSK_REAL_FIELDS_QUALITY(X) "|" FSK_INT_FIELDS(X) FSK_INT_FIELDS_PIPE(X) FSK_INT_FIELDS_QUALITY(X)
#undef X
      ;
  uint64_t h = 0xcbf29ce484222325ull;
  for (const char *p = names; *p; p++) h = (h ^ (uint8_t)*p) * 0x100000001b3ull;
  h = (h ^ kZeroLagPairs) * 0x100000001b3ull;
  h = (h ^ kHandLag) * 0x100000001b3ull;
  return h;
}

inline SnapConfig pack_config(const fskhip_config &c) {
  SnapConfig o;
  std::memset(&o, 0, sizeof(o));
  o.sampleRate = c.sampleRate; o.baudRate = c.baudRate; o.markFrequency = c.markFrequency; o.spaceFrequency = c.spaceFrequency;
  o.syncThreshold = c.syncThreshold; o.preFilterBandwidth = c.preFilterBandwidth;
  // (only the bytes in use: what lies behind preambleLen / sfdLen in the caller's struct is not state)
  for (int i = 0; i < FSKHIP_MAX_PATTERN_BYTES; i++) {
    o.preamblePattern[i] = i < c.preambleLen ? c.preamblePattern[i] : 0;
    o.sfdPattern[i] = i < c.sfdLen ? c.sfdPattern[i] : 0;
  }
  o.preambleLen = c.preambleLen; o.sfdLen = c.sfdLen; o.startBits = c.startBits; o.stopBits = c.stopBits; o.parity = c.parity;
  o.agcEnabled = c.agcEnabled != 0; o.adaptiveThreshold = c.adaptiveThreshold != 0;
  return o;
}
inline fskhip_config unpack_config(const SnapConfig &c) {
  fskhip_config o;
  std::memset(&o, 0, sizeof(o));
  o.sampleRate = c.sampleRate; o.baudRate = c.baudRate; o.markFrequency = c.markFrequency; o.spaceFrequency = c.spaceFrequency;
  o.syncThreshold = c.syncThreshold; o.preFilterBandwidth = c.preFilterBandwidth;
  std::memcpy(o.preamblePattern, c.preamblePattern, sizeof(o.preamblePattern));
  std::memcpy(o.sfdPattern, c.sfdPattern, sizeof(o.sfdPattern));
  o.preambleLen = c.preambleLen; o.sfdLen = c.sfdLen; o.startBits = c.startBits; o.stopBits = c.stopBits; o.parity = c.parity;
  o.agcEnabled = c.agcEnabled; o.adaptiveThreshold = c.adaptiveThreshold;
  return o;
}

// A validated snapshot: the header (copied), its record layout and the records in the caller's bytes.
struct Snap {
  SnapHeader h;
  SnapLayout L;
  const unsigned char *rec;
  SnapRecordHost host_part(size_t i) const {
    SnapRecordHost r;
    std::memcpy(&r, rec + i * h.record_bytes, sizeof(r));
    return r;
  }
  fskhip_config config(size_t i) const {
    fskhip_config c = unpack_config(h.cfg0);
    const SnapRecordHost r = host_part(i);
    c.markFrequency = r.markFrequency; c.spaceFrequency = r.spaceFrequency; c.preFilterBandwidth = r.preFilterBandwidth;
    c.adaptiveThreshold = (int32_t)r.adaptiveThreshold;
    return c;
  }
  uint32_t int_word(size_t i, int f) const {   // IF_* word f of record i
    uint32_t w0 = 0, v;
    for (uint32_t k = 0; k < L.n_sec; k++)
      if (L.sec[k].kind == SNAP_IF) w0 = L.sec[k].w0;
    std::memcpy(&v, rec + i * h.record_bytes + 4u * (w0 + (uint32_t)f), 4);
    return v;
  }
};

// 0 and *s filled in, or -1 and the flaw named in msg.  Order: the frame's front with the state-layout stamp between format and
// header_bytes, precision, the geometry, record_bytes against the layout they make, the size against n_streams, the checksum.
inline int snap_image_open(const void *buf, size_t size, Snap *s, char *msg, size_t msg_cap) {
  SnapHeader &h = s->h;
  const auto stamp = [&] {
    if (h.rf_count != RF_COUNT || h.if_count != IF_COUNT || h.fields_hash != fields_hash())
      return image_flaw(msg, msg_cap, "the snapshot's state layout (%u + %u words, stamp %016llx) is another build's (%d + %d words, stamp %016llx)", h.rf_count,
                        h.if_count, (unsigned long long)h.fields_hash, (int)RF_COUNT, (int)IF_COUNT, (unsigned long long)fields_hash());
    return 0;
  };
  if (const int rc = image_open_front("a snapshot", buf, size, kSnapMagic, kSnapFormat, &h, msg, msg_cap, stamp)) return rc;
  if (h.precision != FSKHIP_PRECISION_F32 && h.precision != FSKHIP_PRECISION_F64) return image_flaw(msg, msg_cap, "unknown precision %d in the snapshot", h.precision);
  if (h.amp_cap != 8u * h.d || h.d == 0 || h.d > (1u << 20) || h.wide > 1 || h.frac > 1 || (h.frac && !h.wide))
    return image_flaw(msg, msg_cap, "inconsistent geometry in the snapshot (d %u, amp_cap %u, wide %u, frac %u)", h.d, h.amp_cap, h.wide, h.frac);
  s->L = snap_layout(h.precision, h.d, h.amp_cap, h.wide, h.frac);
  if (h.record_bytes != 4u * s->L.rec_words)
    return image_flaw(msg, msg_cap, "record_bytes %u, but this geometry and precision make records of %u bytes", h.record_bytes, 4u * s->L.rec_words);
  return image_open_back("n_streams", buf, size, h, h.n_streams, &s->rec, msg, msg_cap);
}

}  // namespace fsk
