// fsk_xmodem_scan.h -- XModemTransport's receive grammar as a per-byte state machine, defined once: the burst scan
// (fsk_xmodem.hip) and the resident receiver (fsk_xmodem_rx.hip) both walk their bytes through it.  What it restates:
// the receive checks of src/transports/xmodem/xmodem.ts:233-320 and the table form of src/utils/crc16.ts:21-38.
// Plain C++ as well as HIP (FSK_XM_FN is empty without a device compiler), so that a host program can run the very same
// code over recorded bytes: tests/cpp/xmodem_rx_grammar_check.cpp.  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fskhip_next.h"

#if defined(__HIPCC__)
#define FSK_XM_FN __device__ __forceinline__
#else
#define FSK_XM_FN inline
#endif

namespace fsk {
namespace xm {

constexpr uint32_t kSOH = 0x01, kEOT = 0x04;  // types.ts:29-34

// table[i] = CRC of the single byte i from a zero register: the 8 shift/xor steps of crc16.ts:25-33
FSK_XM_FN uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i << 8;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) : (c << 1);
  return c & 0xFFFFu;
}
// crc ^= byte << 8, then 8 steps == one table step on the high byte
FSK_XM_FN uint32_t crc_step(const uint32_t *table, uint32_t crc, uint32_t byte) {
  return ((crc << 8) & 0xFFFFu) ^ table[((crc >> 8) ^ byte) & 0xFFu];
}

// per-byte state machine of the receive grammar; every lane walks its own bytes front to back
enum : uint32_t { ST_IDLE, ST_SEQ, ST_NSEQ, ST_LEN, ST_PAYLOAD, ST_CRC_HI, ST_CRC_LO, ST_DONE };

struct Scan {
  uint32_t state, status, expected;
  uint32_t seq, nseq, len, k, crc, rx, start;
  uint32_t packets, dropped, consumed, data_len;
  int32_t err_seq, err_len, crc_rx, crc_calc;
  bool accept;
  uint32_t word;  // payload bytes on their way to data[]: stored a dword at a time where the row allows it

  FSK_XM_FN void init(uint32_t expected_seq) {
    state = ST_IDLE; status = FSKHIP_XM_NEED_MORE; expected = expected_seq;
    seq = nseq = len = k = crc = rx = start = 0;
    packets = dropped = consumed = data_len = 0;
    err_seq = err_len = crc_rx = crc_calc = -1;
    accept = false;
    word = 0;
  }

  // assembleData (xmodem.ts:322-333): byte `off` of the stream's assembled payload.  Tentative until the packet's CRC
  // has matched -- only data[0 .. data_len) is meaningful afterwards.  With a 4-byte aligned row the bytes are merged
  // into dwords (one store per 4 bytes); a partial dword is flushed bytewise when its packet ends.
  template <bool DW>
  FSK_XM_FN void put(uint8_t *drow, size_t data_pitch, uint32_t off, uint32_t b, bool last) {
    if (!drow || (size_t)off >= data_pitch) return;
    if (!DW) { drow[off] = (uint8_t)b; return; }
    const uint32_t sh = (off & 3u) * 8u;
    word = (word & ~(0xFFu << sh)) | (b << sh);
    if ((off & 3u) == 3u && (size_t)off < data_pitch) {
      // full dword: bytes before this packet's first byte inside it were written by an earlier flush and are in `word`
      *reinterpret_cast<uint32_t *>(drow + (off & ~3u)) = word;
    } else if (last) {
      for (uint32_t q = off & ~3u; q <= off; q++) drow[q] = (uint8_t)(word >> ((q & 3u) * 8u));
    }
  }

  template <bool DW>
  FSK_XM_FN void byte(const uint32_t *table, uint32_t b, uint32_t pos, uint8_t *drow, size_t data_pitch) {
    switch (state) {
      case ST_IDLE:  // xmodem.ts:238-252
        if (b == kEOT) {
          status = FSKHIP_XM_EOT;
          state = ST_DONE;
        } else if (b == kSOH) {
          start = pos;
          state = ST_SEQ;
        }
        consumed = pos + 1;
        break;
      case ST_SEQ:
        seq = b;
        state = ST_NSEQ;
        break;
      case ST_NSEQ:
        nseq = b;
        state = ST_LEN;
        break;
      case ST_LEN: {  // xmodem.ts:266-274, 278, 309, 315
        len = b;
        const uint32_t prev = expected == 1 ? 255u : expected - 1;
        if (seq + nseq != 255u) {
          status = FSKHIP_XM_INVALID_SEQUENCE;
        } else if (seq == expected) {
          accept = true;
        } else if (seq == prev) {
          accept = false;
        } else {
          status = FSKHIP_XM_UNEXPECTED_SEQUENCE;
        }
        if (status != FSKHIP_XM_NEED_MORE) {
          err_seq = (int32_t)seq;
          err_len = (int32_t)len;
          dropped++;
          consumed = pos + 1;
          state = ST_DONE;
        } else {
          k = 0;
          crc = 0xFFFFu;
          state = len ? ST_PAYLOAD : ST_CRC_HI;
        }
        break;
      }
      case ST_PAYLOAD:
        if (accept) {
          put<DW>(drow, data_pitch, data_len + k, b, k + 1 == len);
          crc = crc_step(table, crc, b);
        }
        if (++k == len) state = ST_CRC_HI;
        break;
      case ST_CRC_HI:
        rx = b << 8;
        state = ST_CRC_LO;
        break;
      case ST_CRC_LO:
        rx |= b;
        consumed = pos + 1;
        state = ST_IDLE;
        if (accept) {
          packets++;        // statistics.packetsReceived: counted once the payload is in, before the CRC check (xmodem.ts:280)
          if (rx != crc) {  // xmodem.ts:287-291
            status = FSKHIP_XM_INVALID_CRC;
            err_seq = (int32_t)seq;
            err_len = (int32_t)len;
            crc_rx = (int32_t)rx;
            crc_calc = (int32_t)crc;
            dropped++;
            state = ST_DONE;
          } else {  // xmodem.ts:293-303
            data_len += len;
            expected = (expected % 255u) + 1;
          }
        } else {
          dropped++;  // duplicate: consumed and ignored (xmodem.ts:309-314)
        }
        break;
      default:
        break;
    }
  }

  FSK_XM_FN bool inside_packet() const { return state != ST_IDLE && state != ST_DONE; }

  // The one-reply mode (the resident receiveData(), fsk_xmodem_recv_step.h): the reference awaits the modulation of each ACK /
  // NAK before it reads on (xmodem.ts:242, 259, 307, 314), so a walk in this mode feeds bytes only while owes_reply() is false.
  // True once a step has ended that the receiver answers: an accepted packet or a duplicate (ACK), an error (NAK), an EOT (ACK).
  // A walk that stops there has seen at most one such step: seq / len / start are that packet's, packets + dropped its count.
  FSK_XM_FN bool owes_reply() const { return state == ST_DONE || packets + dropped > 0u; }

  FSK_XM_FN void store(fskhip_xmodem_result *out) const {
    fskhip_xmodem_result r;
    r.status = status;
    r.expected_after = expected;
    r.packets = packets;
    r.dropped = dropped;
    r.consumed = consumed;
    r.data_len = data_len;
    r.err_seq = err_seq;
    r.err_len = err_len;
    r.crc_rx = crc_rx;
    r.crc_calc = crc_calc;
    *out = r;
  }

  // the end of a recorded burst: a packet cut by it is charged as FSKHIP_XM_TRUNCATED
  FSK_XM_FN void finish(fskhip_xmodem_result *out) {
    if (inside_packet()) {  // ran out of bytes inside a packet (the reference's wait times out)
      status = FSKHIP_XM_TRUNCATED;
      // what waitForBytes has taken out of the receive buffer by then (xmodem.ts:475-499): SOH, and the three header
      // bytes once they were all there -- pinned to the real XModemTransport by tests/golden/manifest_next.json
      consumed = state >= ST_PAYLOAD ? start + 4u : start + 1u;
      if (state >= ST_PAYLOAD) {
        err_seq = (int32_t)seq;
        err_len = (int32_t)len;
      }
    }
    store(out);
  }

  // the end of what a live line has delivered so far, n bytes: a packet cut by it waits -- the result is that of the
  // bytes before its SOH, and it stays in the receive buffer, SOH included; an error clears the buffer (xmodem.ts:256-259);
  // otherwise what the grammar consumed leaves it (bytes behind an EOT stay).  Returns the bytes to take out.
  FSK_XM_FN uint32_t finish_streaming(fskhip_xmodem_result *out, uint32_t n) {
    uint32_t removed;
    if (inside_packet()) {
      consumed = start;   // (status is NEED_MORE and the error fields -1: nothing of this packet has been charged yet)
      removed = start;
    } else if (status == FSKHIP_XM_INVALID_SEQUENCE || status == FSKHIP_XM_INVALID_CRC || status == FSKHIP_XM_UNEXPECTED_SEQUENCE) {
      removed = n;
    } else {
      removed = consumed;
    }
    store(out);
    return removed;
  }
};

}  // namespace xm
}  // namespace fsk
