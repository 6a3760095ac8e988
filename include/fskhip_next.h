/*
 * fskhip_next.h -- C ABI of libfskhip.so for the rows either side of the demodulator hot path
 * (SURVEY.md 8(f)): the FSKProcessor streaming contract (RX byte ring, ChunkedModulator slice feeder,
 * one process() per 128-sample quantum), CRC-16-CCITT + XModem packet build/validation over the
 * demodulated bytes, and the FIR half of dsp/filters.ts.  Same conventions as fskhip.h: plain pointers
 * and sizes, FSKHIP_OK or a negative FSKHIP_E_* code, fskhip_last_error() for the text, no CPU fallback.
 */
#ifndef FSKHIP_NEXT_H
#define FSKHIP_NEXT_H

#include "fskhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (one number space with fskhip.h's enum, whose values run on at -9: every FSKHIP_E_* has a value of its own, tests/test_abi.py) */
#define FSKHIP_E_BUSY (-8) /* reference: throws 'Modulation already in progress' fsk-processor.ts:90-92 */

/* ---------------------------------------------------------------------------------------------------
 * CRC-16-CCITT and XModem packets (src/utils/crc16.ts, src/transports/xmodem/packet.ts, types.ts,
 * the receive checks of xmodem.ts:233-320) -- batch, one row per stream / packet.
 * The _device forms take device pointers, run on the CURRENT HIP device, asynchronously on `hip_stream`;
 * the _host forms take host pointers, run on `device` and are synchronous.
 * ------------------------------------------------------------------------------------------------- */

/* CRC16.calculate(data) (crc16.ts:21-38: poly 0x1021, init 0xFFFF, no final xor, MSB first) of
 * data[r*pitch .. + lens[r]) for every row r. */
int fskhip_crc16_device(const uint8_t *d_data, size_t pitch, const uint32_t *d_lens, uint32_t n_rows,
                        uint16_t *d_crc, void *hip_stream);
int fskhip_crc16_host(int device, const uint8_t *data, size_t pitch, const uint32_t *lens, uint32_t n_rows,
                      uint16_t *crc);

/* XModemPacket.serialize(XModemPacket.createData(seq, payload)) (packet.ts:21-54) per row:
 * SOH | seq | ~seq | len | payload | crc_hi | crc_lo into out[r*out_pitch ...], out_lens[r] = len + 6.
 * createData's argument checks (sequence 1-255, payload <= 255 bytes) are reported per row as out_lens[r] = 0;
 * the _host form returns FSKHIP_E_INVALID with the reference's message for the first such row. */
int fskhip_xmodem_serialize_device(const uint8_t *d_payloads, size_t payload_pitch, const uint32_t *d_lens,
                                   const uint32_t *d_seqs, uint32_t n_rows, uint8_t *d_out, size_t out_pitch,
                                   uint32_t *d_out_lens, void *hip_stream);
int fskhip_xmodem_serialize_host(int device, const uint8_t *payloads, size_t payload_pitch, const uint32_t *lens,
                                 const uint32_t *seqs, uint32_t n_rows, uint8_t *out, size_t out_pitch,
                                 uint32_t *out_lens);

/* How a scan of one burst ended. */
enum {
  FSKHIP_XM_NEED_MORE = 0,           /* ran out of bytes between packets (the reference would wait / time out) */
  FSKHIP_XM_EOT = 1,                 /* EOT seen where a packet could start (xmodem.ts:241-244) */
  FSKHIP_XM_TRUNCATED = 2,           /* ran out of bytes inside a packet (the reference's waitForBytes times out) */
  FSKHIP_XM_INVALID_SEQUENCE = 3,    /* (seq + nseq) != 255            'Invalid sequence number' xmodem.ts:270-274 */
  FSKHIP_XM_INVALID_CRC = 4,         /* CRC16(payload) != received CRC 'Invalid CRC'             xmodem.ts:287-291 */
  FSKHIP_XM_UNEXPECTED_SEQUENCE = 5  /* neither expected nor previous  'Unexpected sequence number' xmodem.ts:315-319 */
};

typedef struct fskhip_xmodem_result {
  uint32_t status;         /* FSKHIP_XM_* */
  uint32_t expected_after; /* receive.expectedSequence after the scan (xmodem.ts:303) */
  uint32_t packets;        /* statistics.packetsReceived: packets with the expected sequence whose payload + CRC arrived
                              (counted before the CRC check, xmodem.ts:280, so a bad-CRC packet is in it) */
  uint32_t dropped;        /* statistics.packetsDropped increments: bad seq pair / CRC / duplicate / unexpected */
  uint32_t consumed;       /* bytes taken out of the receive buffer (xmodem.ts:475-499): everything up to the end of the last
                              complete step; inside a truncated packet SOH (+ the 3 header bytes once complete) */
  uint32_t data_len;       /* bytes of assembled payload written (true size, even beyond data_pitch) */
  int32_t err_seq;         /* header of the packet that ended the scan with an error / truncation, else -1 */
  int32_t err_len;
  int32_t crc_rx;          /* FSKHIP_XM_INVALID_CRC: received and computed CRC, else -1 */
  int32_t crc_calc;
} fskhip_xmodem_result;

/*
 * XModemTransport's receive grammar (receiveAllPackets / receiveAndProcessPacket, xmodem.ts:233-320) over a
 * recorded burst per stream -- bytes[s*pitch .. + counts[s]) as the demodulator returned them: bytes other than
 * SOH/EOT between packets are ignored; SOH seq nseq len payload crc16 is accepted when seq is the expected
 * sequence and the CRC matches (payload appended to data[s*data_pitch ...], assembleData 322-333; expected
 * advances 1..255,1..), consumed-and-dropped when seq is the previous sequence (duplicate), and ends the scan
 * with an error status otherwise -- where the reference throws, NAKs and clears its buffer.
 * expected[s] is read as the starting expectedSequence (1-255) and left untouched; results[s].expected_after
 * carries the new value.
 */
int fskhip_xmodem_scan_device(const uint8_t *d_bytes, size_t pitch, const uint32_t *d_counts,
                              const uint32_t *d_expected, uint32_t n_streams, uint8_t *d_data, size_t data_pitch,
                              fskhip_xmodem_result *d_results, void *hip_stream);
int fskhip_xmodem_scan_host(int device, const uint8_t *bytes, size_t pitch, const uint32_t *counts,
                            const uint32_t *expected, uint32_t n_streams, uint8_t *data, size_t data_pitch,
                            fskhip_xmodem_result *results);

/* ---------------------------------------------------------------------------------------------------
 * FSKProcessor (src/webaudio/processors/fsk-processor.ts) + ChunkedModulator (src/webaudio/
 * chunked-modulator.ts), one instance per stream of an engine, state resident on the device.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_processor fskhip_processor;

/* new FSKProcessor() per stream: demodulatedBuffer = RingBuffer(Uint8Array, rx_capacity) (1024 in the reference,
 * fsk-processor.ts:84), no pending modulation.  The engine must outlive the processor. */
int fskhip_processor_create(fskhip_engine *e, uint32_t rx_capacity, fskhip_processor **out);
int fskhip_processor_destroy(fskhip_processor *p);

/*
 * process(inputs, outputs) for every stream (fsk-processor.ts:152-167): demodulateFrom(input) --
 * fskCore.demodulateData(input) and every returned byte put into the stream's RX ring, overwriting the oldest
 * when full (294-322, utils.ts:38-48) -- then modulateTo(output): zero fill, the next n_out samples of the
 * pending signal, and on completion the modulation is dropped (256-276).  d_in is [n_streams][in_pitch] float32
 * with n_in samples per stream, d_out [n_streams][out_pitch] with n_out; either may be NULL (that half is
 * skipped, like a missing input/output).  FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE also clears the stream's RX ring
 * when its modulation completes, which the reference's 'modulate' message handler does to avoid
 * self-reception (228-235).  FSKHIP_PROC_GRAPH replays the launches of a quantum as one captured hipGraph.
 * Asynchronous on `hip_stream`.
 */
#define FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE 1u
#define FSKHIP_PROC_GRAPH 2u
int fskhip_processor_process_device(fskhip_processor *p, float *d_in, size_t n_in, size_t in_pitch, float *d_out,
                                    size_t n_out, size_t out_pitch, uint32_t flags, void *hip_stream);
int fskhip_processor_process_host(fskhip_processor *p, float *in, size_t n_in, size_t in_pitch, float *out,
                                  size_t n_out, size_t out_pitch, uint32_t flags);
/* What FSKHIP_PROC_GRAPH has done since fskhip_processor_create (ABI 8, an addition; FSKHIP_ABI_VERSION stays 8): quanta that were
 * captured into a new graph, and quanta that replayed the graph of the call before.  A quantum that ran plainly -- no flag, a
 * timing bracket or a trace armed, the fskhip_processor_process_rate_* forms -- counts as neither.  Read only; either pointer may be
 * NULL.  FSKHIP_E_INVALID for a null processor. */
int fskhip_processor_graph_stats(const fskhip_processor *p, uint64_t *captures, uint64_t *replays);

/*
 * process() with either side in a capture format and layout (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): what a trunk or an RTP
 * gateway delivers and takes -- 16-bit PCM, G.711 mu-law / A-law or floats, stream-major or as interleaved frames
 * [sample][channel] -- goes in and comes out as it is, so a quantum crosses PCIe in 1, 2 or 4 bytes per sample and the host neither
 * widens nor transposes.  Formats and layouts are fskhip.h's FSKHIP_SAMPLES_* and FSKHIP_LAYOUT_*, with its formulas, silence
 * values and pitch rules: pitches are in elements; FSKHIP_LAYOUT_STREAM_MAJOR has element (s, t) at s * pitch + t and needs
 * pitch >= n; FSKHIP_LAYOUT_SAMPLE_MAJOR has it at t * pitch + s and needs pitch >= n_streams, and the columns from n_streams on
 * of a wider frame are neither read nor written.  The contract is fskhip_processor_process_*'s: either side may be NULL, zero
 * lengths are legal, the two flags mean what they mean there.
 *   RX  the processor and its engine end in exactly the state fskhip_processor_process_* leaves when handed the floats
 *       decode(d_in): every ring byte and word, every engine state word, the counters, a decimator left mid-pair by an odd n_in.
 *       (One ingest launch widens the quantum into a float tile kept with the processor; the demodulators run on that.)
 *   TX  element (s, t) of d_out is encode(x), x the float fskhip_processor_process_* writes at (s, t) -- the format's silence where
 *       that zero-fills --, and every generator and completion word ends as there.  (The kernel that generates the samples encodes
 *       and stores them: no float tile, no second launch.)
 * FSKHIP_SAMPLES_F32 in stream-major layout on both sides IS fskhip_processor_process_*.  With FSKHIP_PROC_GRAPH the quantum is
 * one linear capture on the caller's stream; formats and layouts are part of what a replay must match.  The _host form keeps
 * narrow staging with the processor: a stream-major side crosses as one 2-D copy of narrow rows, a sample-major side as one copy
 * of n frames (out: n_streams elements per frame, the caller's other columns stay as they are; in: at the caller's frame pitch, so
 * the columns from n_streams on of a wider input frame cross the link with the rest -- the host reads them, the device ignores
 * them: a caller whose frames are much wider than the batch pays for them on PCIe), all on the processor's stream with one
 * synchronise at the end.  FSKHIP_E_INVALID before any device call, in this order: a null processor; an unknown format or
 * layout (the input side first, whether or not the side is NULL); a pitch that is too small (of a side that is not NULL); a
 * pointer that is not aligned to its element.
 */
int fskhip_processor_process_fmt_device(fskhip_processor *p, const void *d_in, int in_format, int in_layout, size_t n_in,
                                        size_t in_pitch, void *d_out, int out_format, int out_layout, size_t n_out,
                                        size_t out_pitch, uint32_t flags, void *hip_stream);
int fskhip_processor_process_fmt_host(fskhip_processor *p, const void *in, int in_format, int in_layout, size_t n_in,
                                      size_t in_pitch, void *out, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                      uint32_t flags);

/*
 * The 'modulate' request (fsk-processor.ts:87-113) for the streams with mask[s] != 0 (mask NULL = all):
 * pendingModulation = new ChunkedModulator(fskCore); startModulation(payload) (chunked-modulator.ts:31-39:
 * the whole signal is generated now; an EMPTY payload leaves the stream with a pending modulator that never
 * produces samples and never completes, as in the reference).  FSKHIP_E_BUSY ('Modulation already in progress')
 * if any selected stream still has one; nothing is started then.
 */
int fskhip_processor_modulate_host(fskhip_processor *p, const uint8_t *payloads, const uint32_t *lens,
                                   size_t payload_pitch, const uint8_t *mask);
/* ChunkedModulator state per stream: pos/total samples (isModulating() = total > 0, getProgress() = pos/total),
 * pending[s] = pendingModulation != null, completed[s] = modulations completed since create.  Any may be NULL. */
int fskhip_processor_tx_state_host(fskhip_processor *p, uint32_t *pos, uint32_t *total, uint8_t *pending,
                                   uint32_t *completed);
/* the 'demodulate' request without the wait (fsk-processor.ts:117-138): remove everything buffered.  counts[s]
 * is the number of bytes removed into out[s*out_pitch ...] (out_pitch >= rx_capacity never overflows). */
int fskhip_processor_rx_drain_host(fskhip_processor *p, uint8_t *out, size_t out_pitch, uint32_t *counts);
/*
 * The same request for the receivers that hold bytes only (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): a compacted drain.
 * What crosses to the caller is the live bytes and two words per selected stream, not n_streams x out_pitch.
 *   selected    stream s is selected when (mask == NULL || mask[s]) and its ring holds at least max(min_len, 1) bytes: min_len lets
 *               a host wait for a whole packet header, or a whole packet, before it pays for a stream.  The selected streams are
 *               listed in ascending order: streams[0 .. n_active).
 *   CSR layout  offsets has n_active + 1 entries -- the caller provides cap_streams + 1 words --, offsets[0] = 0,
 *               offsets[n_active] = n_bytes; the bytes of streams[i] are data[offsets[i] .. offsets[i+1]), oldest first, tightly
 *               packed: exactly what fskhip_processor_rx_drain_host would have returned for that stream.
 *   the rings   the dense drain's effect, for the selected streams only: readIndex advanced by _length modulo the capacity,
 *               _length = 0, writeIndex and the ring bytes untouched.  A stream that is not selected is not touched in any word.
 *   overflow    atomic: if n_active > cap_streams or n_bytes > cap_bytes the call returns FSKHIP_E_OVERFLOW with *n_active and
 *               *n_bytes set to the true sizes and drains NOTHING -- every ring is as it was, the host calls again with room.
 *               Both caps 0 with null lists is therefore a size query.
 *   _device     asynchronous on `hip_stream`, pointers on the processor's device; d_totals takes three words: n_active, n_bytes,
 *               and 1 if the rings were drained, 0 if a cap was too small (the packing kernel reads the totals and stands down
 *               as a whole; the lists are then undefined).  It uses scratch kept with the processor: one such call at a time.
 * FSKHIP_E_INVALID before any device call, in this order: null n_active or n_bytes (_host) / null d_totals (_device); a null
 * streams or offsets with cap_streams != 0, a null data with cap_bytes != 0; a null processor.  FSKHIP_E_UNSUPPORTED when
 * n_streams x rx_capacity exceeds 2^32 - 1 (offsets are 32-bit).  Like the dense drain it makes the processor a used one
 * (fskhip_processor_remap wants a fresh destination), and it is never part of the captured quantum graph.  Never returns -8.
 */
int fskhip_processor_rx_drain_sparse_host(fskhip_processor *p, const uint8_t *mask, uint32_t min_len, uint32_t *streams,
                                          uint32_t *offsets, uint32_t cap_streams, uint8_t *data, size_t cap_bytes,
                                          uint32_t *n_active, uint32_t *n_bytes);
int fskhip_processor_rx_drain_sparse_device(fskhip_processor *p, const uint8_t *d_mask, uint32_t min_len, uint32_t *d_streams,
                                            uint32_t *d_offsets, uint32_t cap_streams, uint8_t *d_data, size_t cap_bytes,
                                            uint32_t *d_totals, void *hip_stream);
/* demodulatedBufferLength of the 'status' reply (fsk-processor.ts:246). */
int fskhip_processor_rx_length_host(fskhip_processor *p, uint32_t *lengths);
/* reset() (fsk-processor.ts:140-146): RX ring cleared, pending modulation dropped; stream < 0 = all.  The
 * FSKCore state is NOT reset (the reference does not either). */
int fskhip_processor_reset(fskhip_processor *p, int64_t stream);

/*
 * Processor remapping and snapshots (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): the FSKProcessor row carried through the
 * engine's lifecycle calls -- what the reference's host does by keeping or moving a whole FSKProcessor object together with its
 * FSKCore.  fskhip_remap_streams / fskhip_snapshot_streams / fskhip_restore_streams (fskhip.h) carry the engine; these carry
 * the processor over it.  The host makes the destination engine with those calls, creates a processor over it
 * (fskhip_processor_create, the same rx_capacity), and moves the processor's state with the SAME map.  Synchronous host calls.
 *
 * fskhip_processor_remap: stream i of dst continues the processor of stream map[i] of src exactly as if that FSKProcessor
 * object had been moved -- ring content, writeIndex, readIndex and _length verbatim; whether a modulation is pending (the
 * empty-payload pending modulator that never completes included), its payload bytes and generator state (phase, sample
 * position, bit cursor); the `completed` count -- or starts as new FSKProcessor() where map[i] = -1 (empty ring, nothing
 * pending, completed 0).  A source stream may be named more than once (independent clones); those not named are dropped.
 * src is read only and stays usable.  dst's payload store grows to what the carried payloads need; a captured quantum graph
 * is never carried (FSKHIP_PROC_GRAPH captures afresh on dst).  FSKHIP_E_INVALID, with a message naming the first offending
 * index or field and dst left as it was, unless: arguments non-null and dst != src; n_map == dst's stream count and every entry
 * in range or -1; same device, equal rx_capacity; dst freshly created (no process, modulate, drain or reset call yet); the
 * engine of dst stream i has the same fskhip_config as the engine of src stream map[i] (every field: the modulator's frame
 * length and tones come from it, and a pending signal must continue bit for bit).
 *
 * A processor snapshot is a host-side image: plain little-endian bytes, no pointers, every byte defined; two snapshots of the
 * same observable state are byte-identical.  An implementation-versioned checkpoint, not an archive.  Layout:
 *   header, 48 bytes:  u32 magic "FSKP" (0x504B5346) | u32 format (1) | u32 header_bytes (48) | u32 record_bytes |
 *                      u32 n_records | u32 rx_capacity | u32 payload_capacity | u32 0 |
 *                      u64 checksum | u64 0
 *     record_bytes = 64 + payload_capacity + rx_capacity rounded up to a multiple of 16; the image is header_bytes +
 *     n_records x record_bytes long.  checksum: the stream snapshot's function -- over the image's little-endian u64 words w
 *     with the checksum field taken as 0:  a += w, b += a  (mod 2^64);  checksum = a * 0x9E3779B97F4A7C15 ^ b.
 *   records, stream-major, in selection order:
 *     bytes  0..15   u32 writeIndex | u32 readIndex | u32 _length | u32 pendingModulation (0 / 1)
 *     bytes 16..31   u32 completed | u32 samplePosition | u32 totalSamples (0: no signal) | u32 payload length
 *     bytes 32..47   u32 samples into the current bit | u32 bit index | u32 current bit | u32 0
 *     bytes 48..63   f64 phase | u64 0
 *     then payload_capacity bytes of payload, then the ring (rx_capacity bytes, zeros up to the multiple of 16).
 *   canonical form: ring bytes outside the live span [readIndex, readIndex + _length) (modulo rx_capacity) are zero; payload
 *     bytes beyond the pending payload's length are zero; the seven generator words and the phase of a stream without a live
 *     signal (not pending, or pending with totalSamples 0) are zero; payload_capacity is the longest pending payload among the
 *     selected streams rounded up to 16 -- not whatever the source's payload store had grown to.
 *
 * fskhip_processor_snapshot_bytes  the bytes a snapshot of the selected streams takes (it depends on their pending payloads, so
 *                           it takes the selection, not its size; synchronises with p's work).  0 for a null processor.
 * fskhip_processor_snapshot write streams sel[0 .. n_sel) of p (sel NULL: all, in order; a stream may be named more than once)
 *                           into buf.  Synchronises with p's outstanding work; p is read only and stays usable.  *written (may
 *                           be NULL) receives the size; cap too small: FSKHIP_E_OVERFLOW, *written = the size needed.
 * fskhip_processor_snapshot_info_get  what an image holds -- on the host, no device needed -- after validating it: magic,
 *                           format, sizes, checksum, and every record's index words against the capacities.  Each flaw is
 *                           FSKHIP_E_INVALID with a message that names it.
 * fskhip_processor_restore  fskhip_processor_remap with the image standing in for src: map[i] names a RECORD, or is -1.  The
 *                           same-device condition is dropped.  The config condition cannot be checked from the image and is
 *                           the caller's duty: restore dst's engine from the stream snapshot taken at the same moment, with the
 *                           same map (fskhip_restore_streams checks the configs).  Every other precondition of the remap
 *                           applies; everything is validated before anything is written, a refused call leaves dst as it was.
 * fskhip_processor_snapshot_concat  (ABI 8, an addition) host only, no device needed: out = the records of bufs[0], then bufs[1],
 *                           ... under one header -- fskhip_snapshot_concat's contract (fskhip.h) for processor images, and what
 *                           lets the shards of a sharded batch (one processor per GPU) stand as one image, beside the stream
 *                           snapshots' concatenation, so that a live receiver moves from one GPU's processor to another's.
 *                           Every part is validated as fskhip_processor_snapshot_info_get validates it (a flaw: FSKHIP_E_INVALID,
 *                           the message names it and the part); parts of differing rx_capacity are refused.  The result is
 *                           canonical: payload_capacity is per image the longest pending payload of ITS records rounded up
 *                           to 16, so the parts of one batch differ in it as their payloads do -- the result takes the largest
 *                           and every record is written at that pitch, zeros behind the shorter payloads.  The concatenation
 *                           of the shards' images is therefore byte for byte the image one processor holding the same streams
 *                           writes.  *written (may be NULL) receives the size; out NULL or cap too small (cap 0: the size
 *                           query): FSKHIP_E_OVERFLOW, nothing written.  n == 0 or a null array: FSKHIP_E_INVALID.  out
 *                           overlaps no part.
 * Large batches cross in slabs of 8192 streams, as stream snapshots do.  None of these calls returns -8.
 */
typedef struct fskhip_processor_snapshot_info {
  uint32_t n_streams;          /* records in the image */
  uint32_t rx_capacity;
  uint32_t payload_capacity;   /* payload bytes per record */
  uint32_t record_bytes;
} fskhip_processor_snapshot_info;
int fskhip_processor_remap(fskhip_processor *dst, const fskhip_processor *src, const int64_t *map, uint32_t n_map);
size_t fskhip_processor_snapshot_bytes(const fskhip_processor *p, const int64_t *sel, uint32_t n_sel);
int fskhip_processor_snapshot(fskhip_processor *p, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written);
int fskhip_processor_snapshot_info_get(const void *buf, size_t size, fskhip_processor_snapshot_info *info);
int fskhip_processor_snapshot_concat(const void *const *bufs, const size_t *sizes, uint32_t n, void *out, size_t cap, size_t *written);
int fskhip_processor_restore(fskhip_processor *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map);

/* ---------------------------------------------------------------------------------------------------
 * The resident XModem receiver (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): XModemTransport's receive grammar run on the
 * device over a processor's RX rings, in place.  fskhip_xmodem_scan_* judges a recorded burst and charges a packet cut by the
 * burst's end as FSKHIP_XM_TRUNCATED; on a live line the rest of that packet arrives a quantum later.  A receiver keeps what a
 * host would otherwise carry by hand between polls -- expectedSequence and the two running counters per stream -- takes only
 * whole grammar steps out of the rings, and returns the accepted payloads plus one result record for every stream where
 * something happened, in the compacted drain's CSR form.  Raw demodulated bytes do not cross to the host.  The control plane
 * stays with the host: each record says which control bytes the reference would have sent (one ACK per accepted or duplicate
 * packet, a NAK on an error status, the final ACK on FSKHIP_XM_EOT); retries and timeouts are the host's.
 *
 * State per stream, kept with this handle and NOT in the processor (its images and remaps do not carry it; fskhip_xmodem_rx_remap,
 * _snapshot and _restore below do): `expected`
 * (receive.expectedSequence, starts at 1), `packets` and `dropped` (running statistics.packetsReceived / packetsDropped, start
 * at 0, counted as in fskhip_xmodem_result).  fskhip_xmodem_rx_reset is initializeReceive() (xmodem.ts:221-225) for one stream
 * or all (stream < 0): expected = 1 and nothing else -- not the ring, not the counters; what a host calls after FSKHIP_XM_EOT.
 * state_get / state_set carry the three arrays ([n_streams] each, any pointer may be NULL) across a remap or a restore with the
 * host's own map; state_set wants every expected[] in 1..255, else FSKHIP_E_INVALID naming the first bad stream, nothing set.
 * create, reset, state_get and state_set synchronise with the processor's outstanding work.  The processor must outlive every
 * poll, reset and state call of the receiver; fskhip_xmodem_rx_destroy alone may follow the processor's destruction.
 *
 * One poll, for every SELECTED stream -- (mask == NULL || mask[s]) and a ring that holds at least one byte.  L = the live bytes,
 * oldest first ([readIndex, readIndex + _length) modulo the capacity), e = expected[s], scan = fskhip_xmodem_scan_*'s grammar:
 *   1. R = scan(L, e).
 *   2. R.status == FSKHIP_XM_TRUNCATED -- an incomplete packet waits: with c the position of that packet's SOH (R.consumed - 1
 *      before the three header bytes are in, R.consumed - 4 after), the result is R' = scan(L[:c], e) -- FSKHIP_XM_NEED_MORE,
 *      consumed = c, error fields -1 -- and c bytes leave the ring: the packet stays at its front, SOH included, for a later
 *      poll.  FSKHIP_XM_TRUNCATED is never reported by a poll.
 *   3. R.status is INVALID_SEQUENCE, INVALID_CRC or UNEXPECTED_SEQUENCE -- an error ends the scan and clears the ring: R' = R
 *      and all of L leaves (the reference's receive.buffer = [] before its NAK, xmodem.ts:256-259); R'.consumed keeps the
 *      grammar's value, the end of the offending step.
 *   4. otherwise (NEED_MORE or EOT) R' = R and R.consumed bytes leave; bytes behind an EOT stay in the ring.
 *   5. the ring: readIndex advances by the bytes that leave, modulo the capacity, _length shrinks by them; writeIndex and the
 *      ring bytes are untouched.  A stream that is not selected is not touched in any word.
 *   6. the state: expected[s] = R'.expected_after; packets[s] += R'.packets; dropped[s] += R'.dropped.
 *   7. the stream is LISTED when R'.status != FSKHIP_XM_NEED_MORE or R'.packets + R'.dropped > 0 -- when the host has
 *      something to send.  A stream whose poll only swallowed line noise between packets is advanced but not listed.
 * Output: the listed streams in ascending order in streams[0 .. n_events); results[i] = R' of streams[i]; offsets has
 * n_events + 1 entries (the caller provides cap_streams + 1 words), offsets[n_events] = n_bytes; the assembled payload of
 * streams[i] is data[offsets[i] .. offsets[i+1]) -- accepted packets only, in order, no duplicates, nothing of a packet whose
 * CRC failed --, tightly packed.
 * Overflow, as the compacted drain: if n_events > cap_streams or n_bytes > cap_bytes the call returns FSKHIP_E_OVERFLOW with
 * the true sizes and changes NOTHING -- no ring word and no receiver state of any stream, swallowed noise included.  Both caps 0
 * with null lists is therefore a size query.  _device is asynchronous on `hip_stream`, pointers on the processor's device;
 * d_totals takes three words: n_events, n_bytes, and 1 if the poll was committed, 0 if it stood down (the lists are then
 * undefined).  The handle keeps scratch: one poll at a time per handle.
 * FSKHIP_E_INVALID before any device call, in this order: null n_events or n_bytes (_host) / null d_totals (_device); a null
 * streams, results or offsets with cap_streams != 0; a null data with cap_bytes != 0; a null receiver.  create refuses a null
 * processor or a null out.  FSKHIP_E_UNSUPPORTED when n_streams x rx_capacity exceeds 2^32 - 1.  A poll makes the processor a
 * used one, as a drain does, and is never part of the captured quantum graph.  None of these calls returns -8.
 * There is no minimum rx_capacity: a packet that cannot fit its ring waits at the ring's front until the ring's own
 * overwrite-oldest rule pushes it out, exactly as RingBuffer.put would (utils.ts:38-48); rx_capacity >= 261 holds any packet.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_rx fskhip_xmodem_rx;

int fskhip_xmodem_rx_create(fskhip_processor *p, fskhip_xmodem_rx **out);
int fskhip_xmodem_rx_destroy(fskhip_xmodem_rx *r);
int fskhip_xmodem_rx_reset(fskhip_xmodem_rx *r, int64_t stream);
int fskhip_xmodem_rx_state_get(fskhip_xmodem_rx *r, uint32_t *expected, uint32_t *packets, uint32_t *dropped);
int fskhip_xmodem_rx_state_set(fskhip_xmodem_rx *r, const uint32_t *expected, const uint32_t *packets,
                               const uint32_t *dropped);
int fskhip_xmodem_rx_poll_host(fskhip_xmodem_rx *r, const uint8_t *mask, uint32_t *streams, fskhip_xmodem_result *results,
                               uint32_t *offsets, uint32_t cap_streams, uint8_t *data, size_t cap_bytes, uint32_t *n_events,
                               uint32_t *n_bytes);
int fskhip_xmodem_rx_poll_device(fskhip_xmodem_rx *r, const uint8_t *d_mask, uint32_t *d_streams,
                                 fskhip_xmodem_result *d_results, uint32_t *d_offsets, uint32_t cap_streams, uint8_t *d_data,
                                 size_t cap_bytes, uint32_t *d_totals, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------
 * The resident XModem sender (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): XModemTransport.sendData() (xmodem.ts:69-184) for
 * every stream of a processor, with the files, the packet building and the wait's grammar on the device.  The receiver above
 * split the protocol loop -- grammar on the device, timers with the host -- and this is the same split for the send side: a poll
 * looks into the RX rings for the control byte a wait is waiting for, and where one arrived it builds the next packet (or the
 * EOT) on the device and hands it to the processor's modulator, as fskhip_processor_modulate_host would.  No ring byte, no
 * fragment and no packet crosses to the host; what comes back is one event per stream where something happened.  The host keeps
 * the timers: a wait that has lasted too long is ended by naming the stream in the poll's abort mask.
 *
 * What a poll is.  Every wait of the reference's sender calls dataChannel.demodulate(), which returns EVERYTHING buffered; the
 * wait looks at that one reply and throws the rest of it away (waitForControlByte returns the first of ACK / NAK / EOT in the
 * reply, xmodem.ts:413-418; waitForACK succeeds if the reply holds an ACK anywhere, 448-452).  One poll of a ring is one such
 * reply.  The result therefore depends on WHEN the poll happens -- two control bytes found by one poll are one reply, the second
 * is lost; found by two polls they are two replies -- exactly as the reference's result depends on when its message arrives.
 * Unlike the receiver there is NO cut-invariance here, and none is claimed or tested.
 *
 * State per stream, kept with this handle and NOT in the processor (its images and remaps do not carry it; fskhip_xmodem_tx_remap,
 * _snapshot and _restore below do): state (FSKHIP_XT_*),
 * sequence (send.sequence, 1..255), fragment_index, retries (the counter local to withRetry, xmodem.ts:608: it restarts at 0 for
 * every fragment; send.retries plays no part on the send path), packets_sent (statistics.packetsSent: data packets and the EOT)
 * and retransmitted (statistics.packetsRetransmitted); and the stream's file, in one packed store on the device.
 *
 * fskhip_xmodem_tx_create   max_payload_size is config.maxPayloadSize, 1..255 (the reference's default is 128), max_retries is
 *                           config.maxRetries (the reference's default is 10).  Grows the processor's payload store to hold
 *                           max_payload_size + 6 bytes, so that no poll allocates; synchronises with the processor's work.
 * fskhip_xmodem_tx_send_host  sendData(data) for the streams with (mask == NULL || mask[s]): the file of stream s is
 *                           data[offsets[s] .. offsets[s+1]) (offsets has n_streams + 1 entries; those of unselected streams are
 *                           not looked at, except that every selected stream needs offsets[s] <= offsets[s+1]).  ensureIdle first:
 *                           if any selected stream is not FSKHIP_XT_IDLE the call returns FSKHIP_E_BUSY with the reference's text,
 *                           'Transport busy: sendData cannot start while in SENDING_WAIT_ACK state' (the state's own name:
 *                           SENDING_WAIT_NAK, SENDING_WAIT_ACK or SENDING_WAIT_FINAL_ACK) followed by ' (stream N)', and starts
 *                           nothing.  Then initializeSend: sequence 1, fragment_index 0, retries 0, n_fragments =
 *                           max(1, ceil(len / max_payload_size)) -- an empty file is ONE empty fragment --, state WAIT_NAK.
 *                           Nothing is transmitted yet.  A stream's earlier file is replaced; the store is compacted when it has
 *                           to grow.  FSKHIP_E_UNSUPPORTED if the files together would exceed 2^32 - 1 bytes.
 * fskhip_xmodem_tx_reset    reset() (xmodem.ts:370-383) for one stream or all (stream < 0): FSKHIP_XT_IDLE, sequence 1,
 *                           fragment_index 0, retries 0, the file dropped (n_fragments 0), and -- as super.reset() does -- both
 *                           counters 0.  The ring and a pending modulation are left alone.
 * fskhip_xmodem_tx_state_get / _state_set  the six arrays ([n_streams] each, any pointer may be NULL), to carry a sender across
 *                           a remap or a restore: send_host on the new handle, then state_set.  state_set validates everything
 *                           before it sets anything, with the values given taking the place of the current ones: state <= 3,
 *                           sequence in 1..255, and for a stream in WAIT_NAK or WAIT_ACK fragment_index < n_fragments (so a file
 *                           must have been given); FSKHIP_E_INVALID names the first bad stream.
 * create, send_host, reset, state_get and state_set synchronise with the processor's outstanding work.  The processor must outlive
 * every call but fskhip_xmodem_tx_destroy.
 *
 * One poll.  A stream is SELECTED when (mask == NULL || mask[s]) and its state is not FSKHIP_XT_IDLE.  It follows the first of
 * rules 1-3 that applies, and within rule 3 the first branch that matches:
 *   1. abort[s] (abort may be NULL: none): status ABORTED, state IDLE.  This is the wait's timeout: its signal is aborted, every
 *      wait throws, withRetry and waitForInitialNAK do not retry an abort (xmodem.ts:115, 617), sendData fails with 'Operation
 *      aborted' ('Operation aborted at sendData' in the first wait).  The ring and any pending modulation are left alone (the
 *      reference has no cancel).  The "standalone mode" branch and the EOT retry of the reference are not reachable this way, so
 *      the device needs no timer and retransmits no EOT.
 *   2. the processor's tx_pending[s] != 0: nothing happens, the stream is not listed and its ring is not touched -- the reference
 *      is still inside `await modulate()` and is not waiting yet.
 *   3. otherwise L = the live ring bytes, oldest first, is the reply.  ALL of L leaves the ring: readIndex advances by _length
 *      modulo the capacity, _length = 0; writeIndex and the ring bytes are untouched.  An empty L is a legal, empty reply.
 *      WAIT_NAK       c = the first ACK / NAK / EOT of L.  NAK: fragment 0 (fragment_index) is transmitted, state WAIT_ACK.  ACK or
 *                     EOT: returned and skipped, same state (control = c).  None: nothing.
 *      WAIT_ACK       c as above.  ACK: retries = 0, fragment_index++, sequence = sequence % 255 + 1; the next fragment is
 *                     transmitted, or after the last one EOT is, and the state is WAIT_FINAL_ACK.  NAK: retransmitted++; then
 *                     ++retries > max_retries ends the transfer -- status MAX_RETRIES, state IDLE, nothing sent ('Timeout - max
 *                     retries exceeded') --, otherwise retransmitted++ again (an answered NAK counts twice, xmodem.ts:146, 155)
 *                     and the same fragment is transmitted again.  EOT: ignored, the wait goes on (control = EOT).
 *      WAIT_FINAL_ACK an ACK anywhere in L: status DONE, state IDLE, control = ACK.  Anything else, the echo of the sender's own
 *                     EOT and a NAK included, is ignored (control = -1).
 *      Every transmission counts in packets_sent.  A transmission is the 'modulate' request of that stream: the packet
 *      SOH seq ~seq len payload crc_hi crc_lo (CRC-16 of the payload only), or the single byte 0x04, built on the device and
 *      started as fskhip_processor_modulate_host starts it; tx_pending was 0, so it cannot be busy.
 * The event: status, state_after, control (the byte the wait returned, else -1), sent_len (bytes handed to the modulator: 0, 1
 * for EOT, len + 6 for a packet), and sequence, fragment_index, n_fragments, retries after the poll (retries is max_retries + 1
 * after MAX_RETRIES).  A stream is LISTED when status != PROGRESS, or sent_len != 0, or control != -1.  A stream whose reply held
 * only other bytes is drained and not listed.  A stream that is not selected is not touched in any word.
 * Output: the listed streams in ascending order in streams[0 .. n_events), events[i] that of streams[i].
 * Overflow, as the receiver's: if n_events > cap_streams the call returns FSKHIP_E_OVERFLOW with the true count and changes
 * NOTHING -- no ring word, no sender word, no modulation.  cap_streams 0 with null lists is therefore a size query.  _device is
 * asynchronous on `hip_stream`, pointers on the processor's device; d_totals takes three words: n_events, 0, and 1 if the poll
 * was committed, 0 if it stood down (the lists are then undefined).  The handle keeps scratch: one poll at a time per handle.
 * FSKHIP_E_INVALID before any device call, in this order.  poll: null n_events (_host) / null d_totals (_device); a null streams or
 * events with cap_streams != 0; a null sender.  create: a null processor or a null out; max_payload_size outside 1..255.
 * send_host: null offsets; a null sender; then, stream by stream, offsets[s] > offsets[s+1], a file with null data, a stream that
 * is busy (FSKHIP_E_BUSY).  state_get, state_set, reset: a null sender (reset: then a stream out of range).  A poll makes the
 * processor a used one, as a drain does, and is never part of the captured quantum graph.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_tx fskhip_xmodem_tx;
enum { FSKHIP_XT_IDLE = 0, FSKHIP_XT_WAIT_NAK = 1, FSKHIP_XT_WAIT_ACK = 2, FSKHIP_XT_WAIT_FINAL_ACK = 3 };   /* state */
enum { FSKHIP_XT_PROGRESS = 0, FSKHIP_XT_DONE = 1, FSKHIP_XT_MAX_RETRIES = 2, FSKHIP_XT_ABORTED = 3 };        /* status */
typedef struct fskhip_xmodem_tx_event {
  uint32_t status, state_after;
  int32_t  control;        /* the byte that the wait returned (0x06 / 0x15 / 0x04), else -1 */
  uint32_t sent_len;       /* bytes handed to the modulator by this poll: 0, 1 (EOT) or len + 6 */
  uint32_t sequence, fragment_index, n_fragments, retries;   /* after the poll */
} fskhip_xmodem_tx_event;

int fskhip_xmodem_tx_create(fskhip_processor *p, uint32_t max_payload_size, uint32_t max_retries, fskhip_xmodem_tx **out);
int fskhip_xmodem_tx_destroy(fskhip_xmodem_tx *t);
int fskhip_xmodem_tx_send_host(fskhip_xmodem_tx *t, const uint8_t *mask, const uint64_t *offsets, const uint8_t *data);
int fskhip_xmodem_tx_poll_host(fskhip_xmodem_tx *t, const uint8_t *mask, const uint8_t *abort, uint32_t *streams,
                               fskhip_xmodem_tx_event *events, uint32_t cap_streams, uint32_t *n_events);
int fskhip_xmodem_tx_poll_device(fskhip_xmodem_tx *t, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams,
                                 fskhip_xmodem_tx_event *d_events, uint32_t cap_streams, uint32_t *d_totals, void *hip_stream);
int fskhip_xmodem_tx_state_get(fskhip_xmodem_tx *t, uint32_t *state, uint32_t *sequence, uint32_t *fragment_index,
                               uint32_t *retries, uint32_t *packets_sent, uint32_t *retransmitted);
int fskhip_xmodem_tx_state_set(fskhip_xmodem_tx *t, const uint32_t *state, const uint32_t *sequence,
                               const uint32_t *fragment_index, const uint32_t *retries, const uint32_t *packets_sent,
                               const uint32_t *retransmitted);
int fskhip_xmodem_tx_reset(fskhip_xmodem_tx *t, int64_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The resident XModem file receiver (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): XModemTransport.receiveData()
 * (xmodem.ts:186-335) for every stream of a processor.  fskhip_xmodem_rx above runs the receive grammar and leaves ACK / NAK,
 * the retry counter and the file to the host; this handle keeps all of them on the device, with the split the sender uses:
 * grammar, state, file and transmissions on the device, the timers with the host, as masks.  During a transfer only events
 * cross to the host, one record per stream where something happened; the assembled file is read once, at the end.
 * fskhip_xmodem_rx is unchanged and stays the tool for a host that wants the bytes poll by poll.
 *
 * State per stream, kept with this handle and NOT in the processor (fskhip_xmodem_recv_remap, _snapshot and _restore below carry
 * it): state (FSKHIP_XR_*, the reference's RECEIVING_* names),
 * expected (receive.expectedSequence, 1..255), retries (send.retries, which receiveAllPackets counts), file_len,
 * packets_received and dropped (statistics.packetsReceived / packetsDropped, counted as fskhip_xmodem_result counts them),
 * packets_sent (every control byte transmitted); and the stream's file, a row of file_capacity bytes on the device.
 *
 * fskhip_xmodem_recv_create   file_capacity: bytes of file store per stream; max_retries: config.maxRetries.  Grows the
 *                             processor's payload store to hold 1 byte where needed and sizes the _host form's
 *                             staging for n_streams events, so that no poll allocates.
 *                             FSKHIP_E_UNSUPPORTED when n_streams x file_capacity or n_streams x rx_capacity exceeds 2^32 - 1.
 * fskhip_xmodem_recv_start_host  receiveData() up to its first wait for the streams with (mask == NULL || mask[s]).  ensureIdle
 *                             first: if any selected stream is not FSKHIP_XR_IDLE the call returns FSKHIP_E_BUSY with the
 *                             reference's text, 'Transport busy: receiveData cannot start while in RECEIVING_WAIT_BLOCK state'
 *                             (the state's own name) followed by ' (stream N)', and starts nothing.  If a selected stream has
 *                             tx_pending != 0: FSKHIP_E_BUSY, 'Modulation already in progress (stream N)', nothing started.
 *                             Then initializeReceive (xmodem.ts:221-225): expected 1, file length 0, retries 0.  The RX ring
 *                             is NOT cleared: the reference clears only its own receive.buffer, and what the channel buffered
 *                             before the call is still delivered.  Then the NAK byte is started on the processor exactly as
 *                             fskhip_processor_modulate_host starts it, packets_sent++, state FSKHIP_XR_SEND_NAK.
 * fskhip_xmodem_recv_reset    reset() (xmodem.ts:370-383) for one stream or all (stream < 0): IDLE, expected 1, retries 0, file
 *                             length 0, the three counters 0.  The ring and a pending modulation are left alone.
 * fskhip_xmodem_recv_state_get / _state_set  the seven arrays ([n_streams] each, any pointer may be NULL): state, expected,
 *                             retries, file_len, packets_received, dropped, packets_sent.  state_set validates everything before
 *                             it sets anything and names the first bad stream: state <= FSKHIP_XR_SEND_ACK, expected in 1..255,
 *                             file_len <= file_capacity.
 * fskhip_xmodem_recv_files_host  the assembled files of streams sel[0 .. n_sel) in CSR form: offsets has n_sel + 1 entries, the
 *                             file of sel[i] is data[offsets[i] .. offsets[i+1]).  Packed on the device into one contiguous
 *                             buffer, which crosses in one copy.  *n_bytes takes the true size; cap_bytes too small returns
 *                             FSKHIP_E_OVERFLOW and copies nothing (offsets are still written), so cap_bytes 0 is a size query.
 *                             Does not change the receiver.  The partial file of a transfer that failed stays readable until
 *                             the next start or reset.
 * fskhip_xmodem_recv_files_set_host  puts files back (file_len included), to carry a receiver across a remap or a restore:
 *                             files_set_host first, then state_set.  Refuses a file longer than file_capacity.
 * All of these synchronise with the processor's outstanding work.  The processor must outlive every call but _destroy.
 * The device cannot see a modulation end: SEND_NAK and SEND_ACK become WAIT_BLOCK LAZILY, at the first poll that finds
 * tx_pending == 0 -- state_get may report SEND_* after the control byte has gone out.
 *
 * One poll.  A stream is SELECTED when (mask == NULL || mask[s]) and its state is not FSKHIP_XR_IDLE.  It follows the first of
 * rules 1-3 that applies (mask, timeout and abort may each be NULL: all, none, none):
 *   1. abort[s]: status ABORTED, state IDLE -- the external signal or reset(): checkAbort ends in 'Operation aborted'.  The ring
 *      and any pending modulation are left alone; the partial file stays.
 *   2. the processor's tx_pending[s] != 0: nothing happens, no word is touched, the stream is not listed -- the reference is
 *      inside `await sendControl()`, where no timer runs; timeout[s] is ignored.
 *   3. otherwise a SEND_* state becomes WAIT_BLOCK, and with L = the live ring bytes, oldest first, the receive grammar
 *      (fskhip_xmodem_scan_host's) runs from expected[s] and STOPS AT THE FIRST STEP THAT OWES A REPLY: the reference awaits
 *      each control byte's modulation before it reads on, so one poll makes at most one transmission per stream.
 *      accepted packet  (CRC matches) payload appended to the file, expected = expected % 255 + 1, retries = 0,
 *                       packets_received++, the bytes through the packet's end leave the ring, ACK is transmitted, state
 *                       SEND_ACK.  If the payload would not fit in file_capacity: status FILE_FULL, state IDLE, nothing
 *                       transmitted, no counter moves and the packet stays in the ring (line noise in front of its SOH has left).
 *                       The reference has no such limit: this is the resident store's own.
 *      duplicate        (the previous sequence) dropped++, its bytes leave, ACK is transmitted; the state stays WAIT_BLOCK
 *                       and retries is untouched (xmodem.ts:309-314).
 *      error            INVALID_SEQUENCE, INVALID_CRC or UNEXPECTED_SEQUENCE: the counters move as fskhip_xmodem_result
 *                       counts them, ALL of L leaves the ring; then ++retries > max_retries ends the transfer -- status
 *                       MAX_RETRIES, state IDLE, nothing sent ('Receive failed after max retries: ...') --, otherwise NAK is
 *                       transmitted.
 *      EOT              where a packet could start: the bytes through it leave, those behind it stay; ACK is transmitted,
 *                       status DONE, state IDLE.  An empty file is a legal result.
 *      no such step     line noise in front of an incomplete packet leaves, the packet stays at the ring's front, SOH included.
 *                       With timeout[s] the wait's timer has fired: the whole ring is cleared and the ++retries rule above
 *                       follows (NAK or MAX_RETRIES).  A timeout flag on a stream that had a reply-owing step is ignored.
 *      Every transmission counts in packets_sent; each is one byte, built on the device and started as
 *      fskhip_processor_modulate_host starts it (tx_pending was 0, so it cannot be busy).
 * The event: status, state_after, control (the byte transmitted, else -1), step (the FSKHIP_XM_* status of the grammar step;
 * NEED_MORE for an accepted packet, a duplicate and a bare timeout), seq and len of the packet concerned (else -1),
 * accepted_len (bytes appended by this poll), file_len, expected and retries after the poll (retries is max_retries + 1 after
 * MAX_RETRIES), crc_rx / crc_calc as in fskhip_xmodem_result.  A stream is LISTED when status != PROGRESS or something was
 * transmitted.  A stream whose poll only swallowed noise is advanced and not listed.  A stream that is not selected is not
 * touched in any word.  Output: the listed streams ascending in streams[0 .. n_events), events[i] that of streams[i].
 * Overflow: if n_events > cap_streams the call returns FSKHIP_E_OVERFLOW with the true count and changes NOTHING -- no ring
 * word, no receiver word, no file byte, no modulation.  cap_streams 0 with null lists is therefore a size query.  _device is
 * asynchronous on `hip_stream`, pointers on the processor's device; d_totals takes three words: n_events, 0, and 1 if the poll
 * was committed, 0 if it stood down.  The handle keeps scratch: one poll at a time per handle.
 * What is invariant: while no error, timeout or abort occurs (duplicates allowed), the sequence of transmissions, the file and
 * every word at quiescence do not depend on where polls fall or on how the bytes were split between them.  Once an error has
 * cleared the ring the result depends on what had arrived at poll time, as it does in the reference.
 * FSKHIP_E_INVALID before any device call, in this order.  poll: null n_events (_host) / null d_totals (_device); a null streams
 * or events with cap_streams != 0; a null receiver.  create: a null processor or a null out.  start_host, state_get, state_set,
 * reset: a null receiver (reset: then a stream out of range).  files_host: null n_bytes; a null sel or offsets with n_sel != 0;
 * a null data with cap_bytes != 0; a null receiver; a sel entry out of range.  files_set_host: a null sel, offsets with
 * n_sel != 0; a null receiver; then, entry by entry, a sel out of range, offsets[i] > offsets[i+1], a file longer than
 * file_capacity, a file with null data.  A poll makes the processor a used one and is never part of the captured quantum graph.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_recv fskhip_xmodem_recv;
enum { FSKHIP_XR_IDLE = 0, FSKHIP_XR_SEND_NAK = 1, FSKHIP_XR_WAIT_BLOCK = 2, FSKHIP_XR_SEND_ACK = 3 };   /* state */
enum { FSKHIP_XR_PROGRESS = 0, FSKHIP_XR_DONE = 1, FSKHIP_XR_MAX_RETRIES = 2, FSKHIP_XR_ABORTED = 3, FSKHIP_XR_FILE_FULL = 4 };   /* status */
typedef struct fskhip_xmodem_recv_event {
  uint32_t status, state_after;
  int32_t  control;        /* the byte transmitted by this poll (0x06 / 0x15), else -1 */
  uint32_t step;           /* FSKHIP_XM_* of the grammar step */
  int32_t  seq, len;       /* of the packet concerned, else -1 */
  uint32_t accepted_len;   /* bytes appended to the file by this poll */
  uint32_t file_len, expected, retries;   /* after the poll */
  int32_t  crc_rx, crc_calc;
} fskhip_xmodem_recv_event;

int fskhip_xmodem_recv_create(fskhip_processor *p, uint32_t file_capacity, uint32_t max_retries, fskhip_xmodem_recv **out);
int fskhip_xmodem_recv_destroy(fskhip_xmodem_recv *r);
int fskhip_xmodem_recv_start_host(fskhip_xmodem_recv *r, const uint8_t *mask);
int fskhip_xmodem_recv_poll_host(fskhip_xmodem_recv *r, const uint8_t *mask, const uint8_t *timeout, const uint8_t *abort,
                                 uint32_t *streams, fskhip_xmodem_recv_event *events, uint32_t cap_streams, uint32_t *n_events);
int fskhip_xmodem_recv_poll_device(fskhip_xmodem_recv *r, const uint8_t *d_mask, const uint8_t *d_timeout, const uint8_t *d_abort,
                                   uint32_t *d_streams, fskhip_xmodem_recv_event *d_events, uint32_t cap_streams,
                                   uint32_t *d_totals, void *hip_stream);
int fskhip_xmodem_recv_state_get(fskhip_xmodem_recv *r, uint32_t *state, uint32_t *expected, uint32_t *retries, uint32_t *file_len,
                                 uint32_t *packets_received, uint32_t *dropped, uint32_t *packets_sent);
int fskhip_xmodem_recv_state_set(fskhip_xmodem_recv *r, const uint32_t *state, const uint32_t *expected, const uint32_t *retries,
                                 const uint32_t *file_len, const uint32_t *packets_received, const uint32_t *dropped,
                                 const uint32_t *packets_sent);
int fskhip_xmodem_recv_reset(fskhip_xmodem_recv *r, int64_t stream);
int fskhip_xmodem_recv_files_host(fskhip_xmodem_recv *r, const uint32_t *sel, uint32_t n_sel, uint64_t *offsets, uint8_t *data,
                                  size_t cap_bytes, uint64_t *n_bytes);
int fskhip_xmodem_recv_files_set_host(fskhip_xmodem_recv *r, const uint32_t *sel, uint32_t n_sel, const uint64_t *offsets,
                                      const uint8_t *data);

/* ---------------------------------------------------------------------------------------------------
 * The resident XModem handles through remap, snapshot and restore (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): what the
 * reference's host does by keeping or moving a whole XModemTransport object with its FSKProcessor.  The engine is carried by
 * fskhip_remap_streams / fskhip_snapshot_streams / fskhip_restore_streams, the processor over it by fskhip_processor_remap /
 * _snapshot / _restore; the host then creates a FRESH XModem handle over the destination processor and moves the handle's state
 * with the SAME map through the calls below.  They never touch the processor.  The words, the sender's packed file store and the
 * file receiver's rows move on the device; no file passes through host memory on a remap, and an image crosses PCIe once.
 * state_get / state_set, send_host and files_host / files_set_host stay as they are.  Synchronous host calls; none returns -8.
 *
 * _remap: stream i of dst continues the handle state of stream map[i] of src exactly as if that stream's XModemTransport object
 * had been moved: every state word verbatim (the file receiver's SEND_* states included: they go on turning into WAIT_BLOCK lazily,
 * the processor remap carries tx_pending), and the stream's file with it.  Where map[i] = -1 the stream starts as a new transport --
 *   rx    expected 1, counters 0
 *   tx    IDLE, sequence 1, fragment_index 0, retries 0, counters 0, no file
 *   recv  IDLE, expected 1, retries 0, file_len 0, counters 0.
 * A source stream may be named more than once: independent clones, their files copied once per clone.  Source streams that are not
 * named are dropped.  src is read only and stays usable.  Which file bytes move: the sender's file whenever the handle holds one,
 * whatever the stream's state (a later state_set may use it), into a store built densely, in stream order, with no dead bytes; of
 * a file receiver's row exactly file_len bytes, for IDLE streams too (the partial file of a failed transfer stays readable) --
 * row bytes beyond file_len are unspecified in dst.
 * FSKHIP_E_INVALID, with a message naming the first offending index or field and dst left as it was -- everything is validated
 * before anything is written -- unless: the arguments are non-null and dst != src; n_map == dst's stream count and every entry is
 * in range or -1; dst and src are on the same device; dst is freshly created (rx: no poll, reset or state_set call yet; tx: no
 * send, poll, reset or state_set; recv: no start, poll, reset, state_set or files_set); tx: max_payload_size is equal on both
 * handles (the fragment boundaries of a running transfer depend on it); recv: every carried file_len <= dst's file_capacity (the
 * capacity may otherwise differ).  max_retries is the new handle's own and is not compared.  tx: carried files, clones counted,
 * that together exceed 2^32 - 1 bytes: FSKHIP_E_UNSUPPORTED.
 * A handle that has been remapped or restored into is STILL fresh: these calls write every stream of dst, so a second remap or
 * restore into the same handle is accepted and replaces the first as a whole (the sender's store included); only the calls listed
 * above end freshness.  Refusals (FSKHIP_E_INVALID, FSKHIP_E_UNSUPPORTED) write nothing.  A call that fails later, with FSKHIP_E_HIP or
 * FSKHIP_E_NOMEM from the device, may leave dst's words partly written: destroy such a handle and create a new one.
 *
 * An XModem snapshot is a host-side image: plain little-endian bytes, no pointers, every byte defined; two snapshots of the same
 * observable state are byte-identical, whatever the sender's store looked like inside (file order, dead bytes, past compactions).
 * An implementation-versioned checkpoint, not an archive.  Three parts, in this order:
 *   header, 48 bytes:  u32 magic "FSKX" (0x584B5346) | u32 format (1) | u32 header_bytes (48) | u32 kind (1 rx, 2 tx, 3 recv) |
 *                      u32 n_records | u32 record_words (rx 4, tx 8, recv 8) | u32 param0 | u32 param1 |
 *                      u64 checksum | u64 file_bytes
 *     param0 / param1: 0 / 0 (rx), max_payload_size / max_retries (tx), file_capacity / max_retries (recv).  file_bytes: the sum of
 *     the records' file lengths (0 for rx).  checksum: the processor snapshot's function over the image's u64 words, with the
 *     checksum field taken as 0.
 *   word table, n_records x record_words u32, one record per selected stream, in selection order:
 *     rx    expected, packets, dropped, 0
 *     tx    state, sequence, fragment_index, retries, packets_sent, retransmitted, file_len, has_file
 *     recv  state, expected, retries, file_len, packets_received, dropped, packets_sent, 0
 *   the files, concatenated tightly in record order (file_bytes in all), then zero padding to a multiple of 16.
 * The whole image is 48 + 4 x n_records x record_words + file_bytes rounded up to 16 bytes long.
 *
 * fskhip_xmodem_snapshot_info_get  what an image holds -- on the host, no device needed -- after validating ALL of it; each flaw is
 *                           FSKHIP_E_INVALID with a message that names it: magic, format, header_bytes, kind, record_words
 *                           against the kind; the size against the formula above; the checksum; the records' file_len summing
 *                           to file_bytes; padding and reserved words zero; and per record -- rx: expected in 1..255; tx: param0
 *                           in 1..255, state <= 3, sequence in 1..255, has_file 0 or 1, file_len 0 where has_file is 0, and in
 *                           WAIT_NAK or WAIT_ACK a file held with fragment_index < max(1, ceil(file_len / param0)); recv:
 *                           state <= 3, expected in 1..255, file_len <= param0.
 * _snapshot_bytes           the bytes a snapshot of the selected streams takes (it depends on their files, so it takes the
 *                           selection).  0 for a null handle.
 * _snapshot                 write streams sel[0 .. n_sel) (sel NULL: all, in order; a stream may be named more than once) into buf.
 *                           Synchronises with the processor's outstanding work; the handle is read only and stays usable.  *written
 *                           (may be NULL) receives the size; cap too small: FSKHIP_E_OVERFLOW with *written = the size needed and
 *                           nothing written, so cap 0 is a size query.
 * _restore                  _remap with the image standing in for src: map[i] names a RECORD, or is -1.  The same-device condition is
 *                           dropped; the image's kind must be the handle's; every other precondition applies with the image's
 *                           param0 in the place of src's; nothing is written before the whole image and map have passed.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_snapshot_info {
  uint32_t kind;        /* 1 rx, 2 tx, 3 recv */
  uint32_t n_streams;   /* records in the image */
  uint32_t param0, param1;
  uint64_t file_bytes;
} fskhip_xmodem_snapshot_info;
int fskhip_xmodem_snapshot_info_get(const void *buf, size_t size, fskhip_xmodem_snapshot_info *info);

int fskhip_xmodem_rx_remap(fskhip_xmodem_rx *dst, const fskhip_xmodem_rx *src, const int64_t *map, uint32_t n_map);
size_t fskhip_xmodem_rx_snapshot_bytes(const fskhip_xmodem_rx *r, const int64_t *sel, uint32_t n_sel);
int fskhip_xmodem_rx_snapshot(fskhip_xmodem_rx *r, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written);
int fskhip_xmodem_rx_restore(fskhip_xmodem_rx *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map);

int fskhip_xmodem_tx_remap(fskhip_xmodem_tx *dst, const fskhip_xmodem_tx *src, const int64_t *map, uint32_t n_map);
size_t fskhip_xmodem_tx_snapshot_bytes(const fskhip_xmodem_tx *t, const int64_t *sel, uint32_t n_sel);
int fskhip_xmodem_tx_snapshot(fskhip_xmodem_tx *t, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written);
int fskhip_xmodem_tx_restore(fskhip_xmodem_tx *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map);

int fskhip_xmodem_recv_remap(fskhip_xmodem_recv *dst, const fskhip_xmodem_recv *src, const int64_t *map, uint32_t n_map);
size_t fskhip_xmodem_recv_snapshot_bytes(const fskhip_xmodem_recv *r, const int64_t *sel, uint32_t n_sel);
int fskhip_xmodem_recv_snapshot(fskhip_xmodem_recv *r, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written);
int fskhip_xmodem_recv_restore(fskhip_xmodem_recv *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map);

/* ---------------------------------------------------------------------------------------------------
 * The resident XModem wait timers (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): the `timeoutMs` timers of sendData() and
 * receiveData(), kept on the device for every stream of a file receiver or a sender, in the clock a streaming engine has: the
 * engine samples it has processed (timeoutMs 3000 is 144 000 samples at 48 kHz).  The polls above leave the timers to the host,
 * as masks; a host can only build those masks by reading state words and ring lengths back on every quantum.  A timer handle
 * builds them on the device instead and feeds them to the handle's own poll, so a transfer recovers from a lost packet without
 * the host looking at any per-stream word.  The polls, their events, the step rules and the image formats are unchanged; the
 * external abort signal stays with the host, as the polls' abort mask.
 *
 * State per stream, kept with the timer handle: waited (engine samples the current wait has lasted, saturating at 2^32 - 1) and
 * mark (bits 0-1: the stage the timer was armed for, 0..2, always 0 for a sender; bit 2, value 4: was-pending).  The handles' own
 * fskhip_xmodem_*_remap, _snapshot and _restore do NOT carry them; the timers have their own calls with the same map
 * (fskhip_xmodem_timer_remap / _snapshot / _restore, below).
 *
 * fskhip_xmodem_timer_create_recv / _create_tx  a timer over a file receiver / a sender, every stream waited 0, mark 0;
 *                           timeout_samples is timeoutMs in engine samples.  Allocates the _host forms' staging for n_streams
 *                           events, so that no poll allocates.  Several timers over one handle are independent.
 * fskhip_xmodem_timer_reset   waited 0, mark 0 for one stream or all (stream < 0).
 * fskhip_xmodem_timer_state_get / _state_set  the two arrays ([n_streams] each, either pointer may be NULL).  state_set validates
 *                           before it sets anything and names the first bad stream: a mark with other bits than these, a
 *                           stage above 2, a stage on a sender's timer.
 * These synchronise with the processor's outstanding work.  The timer must be destroyed BEFORE its receiver or sender; one whose
 * handle was destroyed first refuses every call but _destroy with FSKHIP_E_INVALID.  (Reusing a timer after its own destroy is
 * undefined, as for every handle here.)
 *
 * One timed poll is fire -> the handle's plain poll -> arm.  `elapsed` is the number of engine samples processed since this
 * timer's previous timed poll; the caller knows it from its own process calls.  The timers are QUANTISED TO THE POLLS: time passes
 * only as `elapsed`, so a wait ends at the first poll at or after its deadline.  They are meant for one poll per quantum.
 *   fire, for a stream the poll will select (mask, state not IDLE):
 *     tx_pending[s] != 0        mark |= 4 and nothing else; flag 0 -- the reference is inside `await sendControl()` / `await
 *                               modulate()`, where no timer runs.  Time spent pending never counts.
 *     else, mark & 4 set, or a receiver in SEND_NAK / SEND_ACK: the wait begins at this poll: waited = 0, mark = 0.
 *     else                      waited = min(waited + elapsed, 2^32 - 1).
 *     flag = waited >= timeout_samples.
 *   the poll.  A receiver takes the flags as its timeout mask and `abort` as it is.  A sender takes (flag | abort[s]) as its abort
 *   mask: a sender's timeout is 'Operation aborted' with nothing retried (the sender's rule 1).
 *   arm, only if the poll was committed; a poll that stood down (FSKHIP_E_OVERFLOW, d_totals[2] == 0) has fire's changes undone, so
 *   it changes no word of the timer either.  For a selected stream:
 *     state IDLE after the poll: waited = 0, mark = 0 (pending or not: an abort ends a pending stream too).
 *     otherwise a stream that was pending at fire is left alone, and for the others
 *     receiver   stage = 0 with no live ring byte left, 1 with fewer than 4 (an SOH is at the front), 2 with 4 or more -- the waits at
 *                xmodem.ts:238 / 267 / 279, 311.  waited = 0 if the stream was listed (something was transmitted), or the poll
 *                took bytes out of the ring without listing it (noise ends a waitForByte and the loop arms a new one,
 *                xmodem.ts:247-250), or the stage rose.  Payload bytes that trickle in inside stage 2 do not re-arm.  mark's
 *                stage = stage.
 *     sender     waited = 0 if the event has sent_len != 0 or a status other than PROGRESS, or returned an EOT in WAIT_ACK (each
 *                turn of that loop arms its own timer, xmodem.ts:137-151).  A skipped ACK / EOT in WAIT_NAK, anything in
 *                WAIT_FINAL_ACK and bytes that are no control bytes leave the timer running: one waitAndSkipForControl /
 *                waitForACK keeps one timer (xmodem.ts:111, 174).
 * A stream that is not selected is not touched in any word.  The events, the lists, the overflow rule and d_totals are the plain
 * polls'.  _device queues fire, fskhip_xmodem_*_poll_device and arm on `hip_stream` with no host synchronisation between them;
 * _host is the same with the lists copied back at the end.  The timer keeps scratch, and reads the handle's: one poll at a time
 * per handle, timed or plain.
 * FSKHIP_E_INVALID before any device call.  create: a null handle or out; timeout_samples 0.  The timed polls: the plain polls'
 * refusals in their order with the timer in the handle's place (null n_events / d_totals; a null streams or events with
 * cap_streams != 0; a null timer); then a timer whose handle is gone; a receiver's timer given to the sender's poll or the other
 * way round.  reset, state_get, state_set: a null timer, a timer whose handle is gone (reset: then a stream out of range).
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_timer fskhip_xmodem_timer;
int fskhip_xmodem_timer_create_recv(fskhip_xmodem_recv *r, uint32_t timeout_samples, fskhip_xmodem_timer **out);
int fskhip_xmodem_timer_create_tx(fskhip_xmodem_tx *t, uint32_t timeout_samples, fskhip_xmodem_timer **out);
int fskhip_xmodem_timer_destroy(fskhip_xmodem_timer *w);
int fskhip_xmodem_timer_reset(fskhip_xmodem_timer *w, int64_t stream);
int fskhip_xmodem_timer_state_get(fskhip_xmodem_timer *w, uint32_t *waited, uint32_t *mark);
int fskhip_xmodem_timer_state_set(fskhip_xmodem_timer *w, const uint32_t *waited, const uint32_t *mark);
int fskhip_xmodem_recv_poll_timed_host(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *mask, const uint8_t *abort,
                                       uint32_t *streams, fskhip_xmodem_recv_event *events, uint32_t cap_streams, uint32_t *n_events);
int fskhip_xmodem_recv_poll_timed_device(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort,
                                         uint32_t *d_streams, fskhip_xmodem_recv_event *d_events, uint32_t cap_streams,
                                         uint32_t *d_totals, void *hip_stream);
int fskhip_xmodem_tx_poll_timed_host(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *mask, const uint8_t *abort,
                                     uint32_t *streams, fskhip_xmodem_tx_event *events, uint32_t cap_streams, uint32_t *n_events);
int fskhip_xmodem_tx_poll_timed_device(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort,
                                       uint32_t *d_streams, fskhip_xmodem_tx_event *d_events, uint32_t cap_streams,
                                       uint32_t *d_totals, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------
 * The wait timers through remap, snapshot and restore (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): the last step of carrying a
 * live batch.  The caller carries the engine, the processor over it and the file receiver or the sender (fskhip_xmodem_recv_* /
 * fskhip_xmodem_tx_remap / _snapshot / _restore), creates a FRESH timer over the destination handle and moves the timers' two
 * words with the SAME map through the calls below.  They never touch the handle or the processor.  The words move on the device;
 * an image crosses PCIe once.  Synchronous host calls; _remap, _snapshot and _restore synchronise with the processor's outstanding
 * work, as state_get does (_snapshot_info_get and _snapshot_bytes are host arithmetic).
 *
 * _remap: stream i of dst gets waited and mark of stream map[i] of src, verbatim -- a wait that was 2.9 s into a 3 s timeout goes
 * on from there, and the was-pending bit keeps the time spent inside `await modulate()` from counting.  Where map[i] = -1 the
 * stream gets 0 and 0, a fresh timer.  A source stream may be named more than once: independent clones.  Source streams that are
 * not named are dropped.  src is read only and stays usable.
 * FSKHIP_E_INVALID, with a message naming the first offending index or field and dst left as it was -- everything is validated
 * before anything is written -- unless: the arguments are non-null and dst != src; neither timer's handle has been destroyed;
 * n_map == dst's stream count and every entry is in range or -1; dst and src are of the same kind (both over a file receiver, or
 * both over a sender); dst and src are on the same device; dst is fresh: no timed poll (one that overflowed included: freshness
 * records that a call was made, not its effect), reset or state_set call yet.  timeout_samples is the new timer's own and is not
 * compared.  A timer that has been remapped or restored into is STILL fresh: these calls write every stream of dst, so a second
 * one replaces the first as a whole.  A call that fails later, with FSKHIP_E_HIP or FSKHIP_E_NOMEM from the device, may leave dst's
 * words partly written: destroy such a timer and create a new one.
 *
 * A timer snapshot is a host-side image: plain little-endian bytes, no pointers, every byte defined; two snapshots of the same
 * words are byte-identical.  An implementation-versioned checkpoint, not an archive.
 *   header, 48 bytes:  u32 magic "FSKW" (0x574B5346) | u32 format (1) | u32 header_bytes (48) | u32 kind (2 tx, 3 recv: the XModem
 *                      image's numbers) | u32 n_records | u32 record_words (2) | u32 timeout_samples | u32 0 | u64 checksum | u64 0
 *     (the XModem image's field offsets).  checksum: the processor snapshot's function over the image's u64 words, with the checksum
 *     field taken as 0.
 *   n_records x (u32 waited, u32 mark), one record per selected stream, in selection order; then zero padding to a multiple of 16.
 * The whole image is 48 + 8 x n_records bytes, rounded up to 16.
 *
 * fskhip_xmodem_timer_snapshot_info_get  what an image holds -- on the host, no device needed -- after validating ALL of it; each
 *                           flaw is FSKHIP_E_INVALID with a message that names it: magic (an "FSKX" image is named as an XModem
 *                           handle's snapshot), format, header_bytes, kind in {2, 3}, record_words, timeout_samples != 0, the
 *                           reserved fields zero; the size against the formula above; the checksum; the padding zero; and per
 *                           record what state_set asks: mark a mark, and stage 0 where the kind is tx.
 * _snapshot_bytes           the bytes a snapshot of the selected streams takes.  0 for a null timer.
 * _snapshot                 write streams sel[0 .. n_sel) (sel NULL: all, in order; a stream may be named more than once) into buf.
 *                           The timer is read only, stays usable and stays fresh.  *written (may be NULL) receives the size; cap
 *                           too small: FSKHIP_E_OVERFLOW with *written = the size needed and nothing written, so cap 0 is a size
 *                           query.  FSKHIP_E_INVALID: a null timer, one whose handle is gone, an entry of sel out of range.
 * _restore                  _remap with the image standing in for src: map[i] names a RECORD, or is -1.  The same-device condition
 *                           is dropped; the image's kind must be dst's; the image's timeout_samples is not compared; nothing is
 *                           written before the whole image and map have passed.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_xmodem_timer_snapshot_info {
  uint32_t kind;             /* 2 tx, 3 recv: the numbers fskhip_xmodem_snapshot_info uses */
  uint32_t n_streams;        /* records in the image */
  uint32_t timeout_samples;
  uint32_t reserved;         /* 0 */
} fskhip_xmodem_timer_snapshot_info;
int fskhip_xmodem_timer_snapshot_info_get(const void *buf, size_t size, fskhip_xmodem_timer_snapshot_info *info);
int fskhip_xmodem_timer_remap(fskhip_xmodem_timer *dst, fskhip_xmodem_timer *src, const int64_t *map, uint32_t n_map);
size_t fskhip_xmodem_timer_snapshot_bytes(const fskhip_xmodem_timer *w, const int64_t *sel, uint32_t n_sel);
int fskhip_xmodem_timer_snapshot(fskhip_xmodem_timer *w, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written);
int fskhip_xmodem_timer_restore(fskhip_xmodem_timer *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map);

/* ---------------------------------------------------------------------------------------------------
 * FIR half of src/dsp/filters.ts: FIRFilter (112-167) batched over streams, and the windowed-sinc designs
 * (243-314) + FilterFactory.createFIR* (346-368).
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_fir fskhip_fir;

/* FilterDesign.sincLowpass / sincHighpass / sincBandpass (filters.ts:243-314).  `taps` must hold n_taps + 1
 * doubles (an even n_taps is bumped to the next odd number by sincLowpass, filters.ts:244-246); the number of
 * coefficients written is returned (negative FSKHIP_E_* on error).  Host arithmetic in doubles, like the
 * reference; agreement with V8 is to the last ulp of libm's sin/cos. */
int fskhip_sinc_lowpass(double cutoff, double sampleRate, uint32_t n_taps, double *taps);
int fskhip_sinc_highpass(double cutoff, double sampleRate, uint32_t n_taps, double *taps);
int fskhip_sinc_bandpass(double center, double bandwidth, double sampleRate, uint32_t n_taps, double *taps);

/* new FIRFilter(coefficients) for n_streams independent streams sharing one coefficient set (filters.ts:117-120);
 * delay lines start at zero.  precision: FSKHIP_PRECISION_F64 accumulates output += c[i]*delay[i] in doubles in
 * the reference's order (bit-identical Float32Array output), FSKHIP_PRECISION_F32 uses fp32 FMAs. */
int fskhip_fir_create(int device, const double *taps, uint32_t n_taps, uint32_t n_streams, int precision,
                      fskhip_fir **out);
int fskhip_fir_destroy(fskhip_fir *f);
uint32_t fskhip_fir_streams(const fskhip_fir *f);   /* the n_streams it was created for (0 for NULL); ABI 7 */
/* processBuffer(input) (filters.ts:142-148) for every stream: out[s][t] = f32(sum_i c[i] * x_s[t-i]), the delay
 * line carried across calls.  in/out are [n_streams][pitch] float32 and may not alias: the _device call refuses ranges
 * [p, p + (n_streams - 1) * pitch + n_per_stream) that overlap with FSKHIP_E_INVALID before anything is launched. */
int fskhip_fir_process_device(fskhip_fir *f, const float *d_in, size_t n_per_stream, size_t in_pitch, float *d_out,
                              size_t out_pitch, void *hip_stream);
int fskhip_fir_process_host(fskhip_fir *f, const float *in, size_t n_per_stream, size_t in_pitch, float *out,
                            size_t out_pitch);
/* reset() (filters.ts:153-156) for one stream, or all when stream < 0. */
int fskhip_fir_reset(fskhip_fir *f, int64_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Rate conversion by an integer factor L, on the device: what puts 8 kHz trunk audio (G.711 or 16-bit PCM) in front of an engine
 * that runs at 48 kHz, and behind it.  An interpolator is FIRFilter above run over the zero-stuffed signal, a decimator the same
 * filter with every L-th output kept; both are evaluated polyphase, so neither the zeros nor the dropped outputs are ever made, and
 * the low rate samples are what crosses PCIe.  With c[0 .. n_taps) the taps and x_s[m] stream s's low rate samples counted from
 * the handle's creation or last reset (samples before 0 are 0.0):
 *   up     out_s[t] = f32(sum c[i] * x_s[(t - i) / L]) over the i, ascending, with (t - i) a non-negative multiple of L;
 *          x = the element's value (fskhip.h: FSKHIP_SAMPLES_*, exact).  Interpolation wants taps with a gain of L.
 *   down   y_s[k] = f32(sum_i c[i] * u_s[kL - i]), i ascending; element (s, k) of the output is y_s[k] in the format
 *          (fskhip.h: "The same formats OUT").
 * precision as for fskhip_fir_create: FSKHIP_PRECISION_F64 rounds every product and sum on its own, FSKHIP_PRECISION_F32 uses
 * fp32 FMAs; either way the values are fskhip_fir_process_device's of that precision over the zero-stuffed input, bit for bit
 * (leaving out a product with a stuffed zero can only change a zero's sign).  The handle keeps the last ceil((n_taps - 1) / L)
 * values (up) or n_taps - 1 floats (down) of every stream, so any cut of a stream into calls gives the same samples.
 *
 * Formats, layouts and pitches (in elements) are fskhip.h's: the low rate side is [n_streams][pitch] (FSKHIP_LAYOUT_STREAM_MAJOR) or
 * frames [sample][pitch >= n_streams] (FSKHIP_LAYOUT_SAMPLE_MAJOR) of the format's elements, the high rate side always float32
 * [n_streams][pitch].  Nothing outside the samples of a row, or the n_streams columns of a frame, is written.
 *
 * Refusals, FSKHIP_E_INVALID before any device call, in this order.  create: taps or out NULL; n_streams or n_taps 0; a direction
 * that is neither; a factor outside 1..32; an unknown precision; then n_taps > 4096, FSKHIP_E_UNSUPPORTED as for the FIR.  The
 * up / down calls: a NULL handle; an unknown format, then layout; and for a call with n_in > 0: a NULL buffer; a pitch that is
 * too small (the float side first); a pointer not aligned to its element; then the wrong call for the handle's direction; and for
 * down an n_in that is no multiple of the factor -- the decimation grid is therefore the handle's own, output k of a stream is
 * always at input kL counted from the reset, and no per-stream phase is needed.  A refused call leaves the history as it was.
 * n_in = 0 is FSKHIP_OK and does nothing once the checks that need no samples have passed: handle, format, layout, direction (the
 * wrong call for a handle is refused whatever its length).
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_resampler fskhip_resampler;
enum { FSKHIP_RESAMPLE_UP = 0, FSKHIP_RESAMPLE_DOWN = 1 };

int fskhip_resampler_create(int device, int direction, uint32_t factor, const double *taps, uint32_t n_taps, uint32_t n_streams,
                            int precision, fskhip_resampler **out);
int fskhip_resampler_destroy(fskhip_resampler *r);
uint32_t fskhip_resampler_streams(const fskhip_resampler *r);   /* the n_streams it was created for (0 for NULL) */
uint32_t fskhip_resampler_history(const fskhip_resampler *r);   /* floats of history per stream (0 for NULL) */
/* history to zero for one stream, or all when stream < 0 */
int fskhip_resampler_reset(fskhip_resampler *r, int64_t stream);
/* up: n_in samples per stream at d_src -> n_in * factor floats per stream at d_dst.  Asynchronous on hip_stream. */
int fskhip_resampler_up_device(fskhip_resampler *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch,
                               float *d_dst, size_t dst_pitch, void *hip_stream);
/* down: n_in floats per stream at d_src -> n_in / factor samples per stream at d_dst.  d_lens (device, n_streams words; may be
 * NULL): input element t >= d_lens[s] of stream s reads as 0.0f whatever the row holds there -- also in the history the call
 * leaves --, so a ragged batch rings out and ends in the format's silence.  Asynchronous on hip_stream. */
int fskhip_resampler_down_device(fskhip_resampler *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens,
                                 void *d_dst, int format, int layout, size_t dst_pitch, void *hip_stream);
/* the same with host buffers (lens too), through the handle's own staging slabs and stream; synchronous */
int fskhip_resampler_up_host(fskhip_resampler *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst,
                             size_t dst_pitch);
int fskhip_resampler_down_host(fskhip_resampler *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst,
                               int format, int layout, size_t dst_pitch);
/* the history rows, [n_streams][fskhip_resampler_history()] floats on the host, oldest first: the by-hand carry of a handle across
 * a remap (get, permute the rows, set on a handle of the same direction, factor and taps).  Synchronous; nothing is copied when
 * the history is empty.  fskhip_resampler_remap / _snapshot / _restore below do the same on the device, and a resampler has a
 * snapshot image of its own. */
int fskhip_resampler_state_get(fskhip_resampler *r, float *state);
int fskhip_resampler_state_set(fskhip_resampler *r, const float *state);

/*
 * A resampler through remap, snapshot and restore (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): the handle follows its streams
 * with the SAME map the engine (fskhip_remap_streams ...), the processor (fskhip_processor_remap ...) and the resident XModem
 * handles (fskhip_xmodem_*_remap ...) were carried with, so the cut-invariance of the rate calls holds across a remap.  Unlike
 * those calls, remap and restore CREATE their handle: a resampler's design (direction, factor, taps, precision) is the source's
 * or the image's own, so there is no destination that could disagree.  The rows move on the device.  Synchronous host calls.
 *
 * fskhip_resampler_remap   *out: a new handle on src's device with src's direction, factor, taps and precision, for n_map streams.
 *                          Stream i continues stream map[i] of src: its history row verbatim, every bit (NaN payloads and the sign
 *                          of zero included).  Where map[i] = -1 stream i starts with a zero history, as after reset.  A source
 *                          named several times gives independent clones; sources not named are dropped.  src is read only and
 *                          stays usable.  Destroy *out with fskhip_resampler_destroy.
 * A resampler snapshot is a host-side image: plain little-endian bytes, no pointers, every byte defined.  It is canonical: two
 * handles in the same observable state give the same bytes, whichever way they came to it.  A history is plain floats and the
 * taps are create's doubles, so nothing in an image depends on the build that wrote it; the format number says how to read it.
 *   header, 48 bytes:  u32 magic "FSKR" (0x524B5346) | u32 format (1) | u32 header_bytes (48) | u32 record_bytes (4 x history) |
 *                      u32 n_records | u32 direction | u32 factor | u32 n_taps | u32 precision | u32 history | u64 checksum
 *     history: fskhip_resampler_history() of the design.  checksum: the processor snapshot's function over the image's u64 words,
 *     with the checksum field taken as 0 (the other image formats keep it in the header too).
 *   the taps, n_taps doubles as given to create
 *   the rows, n_records x history floats packed tightly, one per selected stream, in selection order, oldest sample first
 *   zero padding to a multiple of 16 bytes
 * fskhip_resampler_snapshot_bytes  *bytes = the size of an image of n_sel records of this handle.
 * fskhip_resampler_snapshot        write streams[0 .. n_sel) (NULL: all streams, in order, whatever n_sel; a stream may be named more
 *                          than once) into image.  Synchronises with the device's outstanding work; the handle is read only and
 *                          stays usable.  *written (may be NULL) receives the size; cap too small (or image NULL):
 *                          FSKHIP_E_OVERFLOW with *written = the size needed and nothing written, so cap 0 is a size query.
 * fskhip_resampler_restore         remap with the image standing in for src, on any device: map[i] names a RECORD, or is -1; a NULL
 *                          map takes every record, in order (n_map is then ignored).  The design is the image's.
 * fskhip_resampler_snapshot_info_get   what an image holds -- on the host, no device needed -- after validating ALL of it.
 *
 * Refusals, FSKHIP_E_INVALID before any device call, in this order; a refused call creates nothing, leaves *out alone and the
 * source as it was.
 *   remap           src or out NULL; map NULL with n_map > 0; n_map 0; the first map[i] below -1 or not below src's stream count.
 *   snapshot_bytes  r or bytes NULL.
 *   snapshot        r NULL; the first streams[i] below 0 or not below the handle's stream count; then the room (FSKHIP_E_OVERFLOW).
 *   an image        (info_get, restore) NULL; fewer bytes than a header; magic; format; header_bytes; a direction or precision that
 *                   is neither; factor outside 1..32 or n_taps outside 1..4096 (create's limits); a history that does not follow
 *                   from direction, factor and n_taps; record_bytes; the size against the layout above; the checksum; a padding
 *                   byte that is not zero.  info_get then: info NULL.
 *   restore         out NULL; the image; map non-NULL with n_map 0, or a NULL map over an image without records; the first map[i]
 *                   below -1 or not below the image's record count.  Then what create refuses for the device.
 */
typedef struct fskhip_resampler_snapshot_info {
  uint32_t n_streams;   /* records in the image */
  int direction;        /* FSKHIP_RESAMPLE_* */
  uint32_t factor, n_taps;
  int precision;        /* FSKHIP_PRECISION_* */
  uint32_t history;     /* floats per record */
} fskhip_resampler_snapshot_info;
int fskhip_resampler_remap(const fskhip_resampler *src, const int64_t *map, uint32_t n_map, fskhip_resampler **out);
int fskhip_resampler_snapshot_bytes(const fskhip_resampler *r, uint32_t n_sel, size_t *bytes);
int fskhip_resampler_snapshot(const fskhip_resampler *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written);
int fskhip_resampler_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_resampler **out);
int fskhip_resampler_snapshot_info_get(const void *image, size_t bytes, fskhip_resampler_snapshot_info *info);

/*
 * process() with both sides at the trunk's own rate (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): one FSKProcessor quantum whose
 * input is interpolated by `up` and whose output is decimated by `down` on the device, so a 20 ms packet of 8 kHz G.711 goes in
 * and comes out as it is.  n_in, n_out and the pitches count low rate elements; formats, layouts and pitches are fskhip.h's, exactly
 * as fskhip_processor_process_fmt_* take them.  With Lu / Ld the handles' factors the call IS, bit for bit,
 *   fskhip_resampler_up_device(up, d_in, ..., X)  ->  fskhip_processor_process_device(p, X, n_in * Lu, ..., Y, n_out * Ld, ...)
 *   ->  fskhip_resampler_down_device(down, Y, n_out * Ld, ..., d_lens = NULL, d_out, ...):
 * the elements written, every word of processor and engine state and both handles' histories (fskhip_resampler_state_get) end as
 * that chain leaves them, so any cut of a stream into quanta gives the same bytes and the same samples.  A side whose buffer is NULL
 * is absent, as in process(): its handle is ignored (and may be NULL) and its history untouched.
 *   RX  one interpolator launch writes into a float tile kept with the processor, the demodulators run on that.
 *   TX  stream-major: one kernel generates the n_out * Ld samples, keeps them in an LDS delay line, evaluates every Ld-th output
 *       of the decimator's FIR from it, encodes and stores: the high rate floats never reach memory.  A decimator too long for that
 *       delay line (every default design up to factor 12 fits; the limit is a few hundred taps and depends on factor and format),
 *       and interleaved frames, for which that measured faster, take two launches through a float tile kept with the processor,
 *       with the same results.
 * FSKHIP_PROC_GRAPH is ignored: the handles' history buffers change places from call to call, so these forms launch plainly
 * whatever that flag says; FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE means what it means in process().  The _host form stages the low
 * rate samples as fskhip_processor_process_fmt_host stages its own and synchronises at the end.
 * FSKHIP_E_INVALID before any device call, in this order: a null processor; an unknown format, then layout, the input side first
 * (whether or not the side is NULL); for each side that has a buffer, the input side first: a null handle, a handle of the wrong
 * direction, one whose fskhip_resampler_streams is not the processor's, one on another device; a pitch that is too small, in before
 * out; a pointer that is not aligned to its element.  A refused call leaves the processor and both histories as they were.
 */
int fskhip_processor_process_rate_device(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *d_in,
                                         int in_format, int in_layout, size_t n_in, size_t in_pitch, void *d_out, int out_format,
                                         int out_layout, size_t n_out, size_t out_pitch, uint32_t flags, void *hip_stream);
int fskhip_processor_process_rate_host(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *in,
                                       int in_format, int in_layout, size_t n_in, size_t in_pitch, void *out, int out_format,
                                       int out_layout, size_t n_out, size_t out_pitch, uint32_t flags);

/* ---------------------------------------------------------------------------------------------------
 * Rate conversion by a ratio L / M, on the device (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): what puts 44.1 kHz audio -- the
 * common sound-card and WebAudio AudioContext rate -- in front of an engine that runs at 48 kHz (L / M = 160 / 147) and behind it
 * (147 / 160).  A converter has an up factor L and a down factor M, coprime, each in 1..256, and n_taps taps c[].  It is FIRFilter
 * above run over the input zero-stuffed by L with every M-th output kept.  With x_s[m] stream s's input samples counted from the
 * handle's creation or last reset (samples before 0 are 0.0):
 *   y_s[j] = f32(sum over k = 0, 1, ... while p + kL < n_taps of c[p + kL] * x_s[m - k]),  p = (jM) mod L,  m = (jM) div L
 * the k ascending: the FIR's own ascending tap order with the products against stuffed zeros left out.  precision as for
 * fskhip_fir_create: FSKHIP_PRECISION_F64 rounds every product and sum on its own, FSKHIP_PRECISION_F32 uses fp32 FMAs; either way
 * the values are fskhip_fir_process_device's of that precision over the zero-stuffed input, column jM, bit for bit (only a zero's
 * sign may differ).  It is evaluated polyphase: no stuffed zero and no dropped output is ever computed or stored.  Interpolation
 * wants taps with a gain of L.
 *
 * A call takes n_in samples per stream, a multiple of M, and writes n_in / M * L per stream: the output grid is the handle's own,
 * as the decimator's is, and no per-stream phase exists.  The handle keeps the last ceil((n_taps - 1) / L) inputs of every stream,
 * so any cut of a stream into calls of whole multiples of M gives the same samples.
 *
 * The two directions are named for the side that carries the capture format, not for up or down; either may go either way in rate.
 *   FSKHIP_RATECVT_CAPTURE   reads a format and layout of fskhip.h (FSKHIP_SAMPLES_*, exact; [n_streams][pitch] or frames
 *                            [sample][pitch >= n_streams]) and writes float32 rows [n_streams][pitch]: 44.1 kHz in front of the engine.
 *   FSKHIP_RATECVT_PLAYBACK  reads float32 rows and writes the format and layout (fskhip.h: "The same formats OUT"): the engine's
 *                            output towards 44.1 kHz.  d_lens as fskhip_resampler_down_device takes it.
 * Nothing outside the samples of a row, or the n_streams columns of a frame, is written.
 *
 * Refusals, FSKHIP_E_INVALID before any device call, in this order.  create: taps or out NULL; n_streams or n_taps 0; a direction
 * that is neither; up or down outside 1..256; up and down not coprime; an unknown precision; then n_taps > 4096,
 * FSKHIP_E_UNSUPPORTED as for the FIR.  The capture / playback calls: a NULL handle; an unknown format, then layout; and for a call
 * with n_in > 0: a NULL buffer; a pitch that is too small (the float side first); a pointer not aligned to its element; then the
 * wrong call for the handle's direction; an n_in that is no multiple of down.  A refused call leaves the history as it was.
 * n_in = 0 is FSKHIP_OK and does nothing once the checks that need no samples have passed: handle, format, layout, direction.
 * (The NULL handle comes first, so without a device -- where create ends in FSKHIP_E_NO_DEVICE -- only create's refusals and the NULL
 * handle's can be met; tests/test_ratecvt_refusals_cpu.py holds those, tests/test_gpu_ratecvt.py the rest, in this order.)
 * fskhip_ratecvt_state_get / _set are the by-hand carry of a handle; fskhip_ratecvt_remap / _snapshot / _restore ("A rate converter
 * through remap, snapshot and restore", below) do the same on the device, and a converter has a snapshot image of its own.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_ratecvt fskhip_ratecvt;
enum { FSKHIP_RATECVT_CAPTURE = 0, FSKHIP_RATECVT_PLAYBACK = 1 };

int fskhip_ratecvt_create(int device, int direction, uint32_t up, uint32_t down, const double *taps, uint32_t n_taps, uint32_t n_streams,
                          int precision, fskhip_ratecvt **out);
int fskhip_ratecvt_destroy(fskhip_ratecvt *r);
uint32_t fskhip_ratecvt_streams(const fskhip_ratecvt *r);   /* the n_streams it was created for (0 for NULL) */
uint32_t fskhip_ratecvt_history(const fskhip_ratecvt *r);   /* floats of history per stream (0 for NULL) */
/* history to zero for one stream, or all when stream < 0 */
int fskhip_ratecvt_reset(fskhip_ratecvt *r, int64_t stream);
/* capture: n_in samples per stream at d_src -> n_in / down * up floats per stream at d_dst.  Asynchronous on hip_stream. */
int fskhip_ratecvt_capture_device(fskhip_ratecvt *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch,
                                  float *d_dst, size_t dst_pitch, void *hip_stream);
/* playback: n_in floats per stream at d_src -> n_in / down * up samples per stream at d_dst.  d_lens (device, n_streams words; may
 * be NULL): input element t >= d_lens[s] of stream s reads as 0.0f whatever the row holds there -- also in the history the call
 * leaves --, so a ragged batch rings out and ends in the format's silence.  Asynchronous on hip_stream. */
int fskhip_ratecvt_playback_device(fskhip_ratecvt *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens,
                                   void *d_dst, int format, int layout, size_t dst_pitch, void *hip_stream);
/* the same with host buffers (lens too), through the handle's own staging slabs and stream; synchronous */
int fskhip_ratecvt_capture_host(fskhip_ratecvt *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst,
                                size_t dst_pitch);
int fskhip_ratecvt_playback_host(fskhip_ratecvt *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst,
                                 int format, int layout, size_t dst_pitch);
/* the history rows, [n_streams][fskhip_ratecvt_history()] floats on the host, oldest first (get, permute the rows, set on a handle
 * of the same direction, ratio and taps).  Synchronous; nothing is copied when the history is empty. */
int fskhip_ratecvt_state_get(fskhip_ratecvt *r, float *state);
int fskhip_ratecvt_state_set(fskhip_ratecvt *r, const float *state);

/*
 * process() with both sides at a converter's outer rate (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): one FSKProcessor quantum
 * whose input goes through `capture` and whose output through `playback` on the device, so a receiver bank behind sound cards or a
 * WebAudio AudioContext at 44.1 kHz takes and gives its quanta as they are.  n_in and in_pitch count capture rate elements, n_out
 * and out_pitch playback rate elements; n_in is a multiple of capture's down factor Mc, n_out of playback's up factor Lp: whole
 * periods.  The quantum inside is n_in / Mc * Lc engine samples in and n_out / Lp * Mp engine samples out.  Formats, layouts and
 * pitches are fskhip.h's, exactly as fskhip_processor_process_fmt_* take them.  The call IS, bit for bit,
 *   fskhip_ratecvt_capture_device(capture, d_in, ..., X)  ->  fskhip_processor_process_device(p, X, n_in / Mc * Lc, ..., Y, n_out / Lp * Mp, ...)
 *   ->  fskhip_ratecvt_playback_device(playback, Y, n_out / Lp * Mp, ..., d_lens = NULL, d_out, ...):
 * the elements written, every word of processor and engine state and both handles' histories (fskhip_ratecvt_state_get) and
 * ping-pong positions end as that chain leaves them, so any cut of a stream into legal quanta gives the same bytes and the same
 * samples.  A side whose buffer is NULL is absent, as in process(): its handle is ignored (and may be NULL) and its history untouched.
 *   RX  one capture launch writes into a float tile kept with the processor, the demodulators run on that.
 *   TX  stream-major: one kernel generates the engine's samples, keeps them in an LDS delay line of ceil((n_taps - 1) / Lp) + 4
 *       samples per stream, takes every output of the converter's sum from it as soon as its newest input is written, encodes and
 *       stores: the engine rate floats never reach memory.  A converter too long for that delay line (its history beyond some 240
 *       samples per stream; the default 147 / 160 design needs 22), and interleaved frames, take two launches through a float tile
 *       kept with the processor, with the same results.
 * FSKHIP_PROC_GRAPH is ignored, as for the fskhip_processor_process_rate_* forms and for their reason;
 * FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE means what it means in process().  The _host form stages the outer rate samples as
 * fskhip_processor_process_fmt_host stages its own and synchronises at the end.
 * FSKHIP_E_INVALID before any device call, in this order: a null processor; an unknown format, then layout, the input side first
 * (whether or not the side is NULL); for each side that has a buffer, the input side first: a null handle, a handle of the wrong
 * direction, one whose fskhip_ratecvt_streams is not the processor's, one on another device; a pitch that is too small, in before
 * out; a pointer that is not aligned to its element; an n_in that is no multiple of Mc, then an n_out that is no multiple of Lp
 * (each for a side that has a buffer).  A refused call leaves the processor and both histories as they were.
 */
int fskhip_processor_process_ratecvt_device(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *d_in,
                                            int in_format, int in_layout, size_t n_in, size_t in_pitch, void *d_out, int out_format,
                                            int out_layout, size_t n_out, size_t out_pitch, uint32_t flags, void *hip_stream);
int fskhip_processor_process_ratecvt_host(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *in,
                                          int in_format, int in_layout, size_t n_in, size_t in_pitch, void *out, int out_format,
                                          int out_layout, size_t n_out, size_t out_pitch, uint32_t flags);

/*
 * Rate conversion in calls of any length (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): what lets a 128-frame WebAudio render
 * quantum, or a sound card's 256, 441 or 512 frames, go through a converter as they arrive, with no rebuffering to multiples of
 * `down` in front of it.  A handle carries a position pos in 0 .. down - 1, the inputs taken since the last period boundary (a
 * period is `down` inputs and `up` outputs), one word for all its streams: 0 at creation and after fskhip_ratecvt_reset(r, -1);
 * fskhip_ratecvt_reset(r, stream >= 0) leaves it, and that stream goes on as one that has received zeros.  With x_s[m] and y_s[j]
 * as above, counted from the last boundary, a call of n_in inputs per stream from position pos writes the outputs whose newest
 * input (jM) div L lies in the call, in order:
 *   j = ceil(pos * L / M) .. ceil((pos + n_in) * L / M) - 1,   out_count_any(pos, n_in) = ceil((pos + n_in) L / M) - ceil(pos L / M)
 * of them -- n_in / M * L for whole periods, possibly none where L < M (one input at 13 of the 160 positions of 147 / 160); such a
 * call still takes its inputs.  Afterwards the position is (pos + n_in) mod M and the history the last ceil((n_taps - 1) / L) inputs.
 * Every value is the one the whole-period calls give, bit for bit, so any cut of a stream into calls of any lengths gives the same
 * samples, the same history and the same position.  in_count_any(pos, n_out) is the smallest n_in that writes at least n_out:
 * 0 for 0, else floor((ceil(pos L / M) + n_out - 1) M / L) + 1 - pos; it writes exactly n_out whenever L <= M.
 *
 * The four _any calls are fskhip_ratecvt_capture_device / _playback_device / _capture_host / _playback_host without the multiple:
 * the same arguments (d_lens counts from the call's first input), the same refusals in the same order but the last, pitches held
 * to out_count_any, n_in = 0 handled alike; *n_out (may be NULL) is set to the elements per stream a call that is not refused wrote.
 * The four existing calls still refuse an n_in that is no multiple of `down`; they work from whatever position the handle is at
 * and leave it where it was.  fskhip_ratecvt_position / _position_set are the by-hand carry beside fskhip_ratecvt_state_get /
 * _set, whose layout is unchanged; position_set refuses a NULL handle and pos >= down (FSKHIP_E_INVALID).  The two counts answer
 * from the handle's current position (0 for a NULL handle).
 *
 * fskhip_processor_process_ratecvt_device / _host refuse a handle (of a side that has a buffer) whose position is not 0 with
 * FSKHIP_E_INVALID, behind all their other refusals, the capture handle first: their fused TX kernel begins at a period boundary.
 * fskhip_processor_process_ratecvt_any_device / _host take the same arguments with any n_in and n_out.  The call IS, bit for bit,
 *   fskhip_ratecvt_capture_any_device(capture, d_in, ..., n_in, X)  ->  fskhip_processor_process_device(p, X,
 *   fskhip_ratecvt_out_count_any(capture, n_in), ..., Y, fskhip_ratecvt_in_count_any(playback, n_out), ...)  ->
 *   fskhip_ratecvt_playback_any_device(playback, Y, ..., d_lens = NULL, d_out, ...)
 * with a side of the processor call that has 0 engine samples left out (NULL).  TX is the whole-period call's choice: stream-major
 * output through a converter that fits the delay line takes the fused kernel in its any-length form, which starts from the
 * playback handle's position (whole periods from position 0 whose engine count is whole periods too: the whole-period form);
 * interleaved frames and longer converters take the two launches; fskhip_processor_last_tx_kernel says which.  The refusals are the
 * whole-period call's without the two multiples; then, where `up` > `down`, an n_out the playback handle cannot produce from its
 * position -- in_count_any(n_out) inputs write more -- is FSKHIP_E_INVALID, the message naming the counts below and above it that
 * it can produce.  A refused call leaves the processor, both histories and both positions as they were.
 */
int fskhip_ratecvt_capture_any_device(fskhip_ratecvt *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch,
                                      float *d_dst, size_t dst_pitch, size_t *n_out, void *hip_stream);
int fskhip_ratecvt_playback_any_device(fskhip_ratecvt *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens,
                                       void *d_dst, int format, int layout, size_t dst_pitch, size_t *n_out, void *hip_stream);
int fskhip_ratecvt_capture_any_host(fskhip_ratecvt *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch,
                                    float *dst, size_t dst_pitch, size_t *n_out);
int fskhip_ratecvt_playback_any_host(fskhip_ratecvt *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens,
                                     void *dst, int format, int layout, size_t dst_pitch, size_t *n_out);
uint32_t fskhip_ratecvt_position(const fskhip_ratecvt *r);   /* 0 for NULL */
int fskhip_ratecvt_position_set(fskhip_ratecvt *r, uint32_t pos);
size_t fskhip_ratecvt_out_count_any(const fskhip_ratecvt *r, size_t n_in);
size_t fskhip_ratecvt_in_count_any(const fskhip_ratecvt *r, size_t n_out);
int fskhip_processor_process_ratecvt_any_device(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback,
                                                const void *d_in, int in_format, int in_layout, size_t n_in, size_t in_pitch,
                                                void *d_out, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                                uint32_t flags, void *hip_stream);
int fskhip_processor_process_ratecvt_any_host(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *in,
                                              int in_format, int in_layout, size_t n_in, size_t in_pitch, void *out, int out_format,
                                              int out_layout, size_t n_out, size_t out_pitch, uint32_t flags);
/*
 * Which TX path the last quantum ran (ABI 8, additions; FSKHIP_ABI_VERSION stays 8), modelled on fskhip_last_kernel: the name of
 * the kernel that wrote the quantum's output, or of the two launches that stand for one, joined by '+'; "" where the quantum had no
 * TX side (a NULL output or n_out = 0), before the first quantum and for a NULL processor.  Every process form sets it behind a
 * quantum it has issued; a call that is refused, or that fails before or in a launch, leaves it:
 *   fskhip_processor_process_*          "processor_io_kernel"
 *   fskhip_processor_process_fmt_*      "processor_io_fmt_kernel" ("processor_io_kernel" for float32 stream-major output)
 *   fskhip_processor_process_rate_*     "processor_io_rate_kernel" or "processor_io_kernel+resample_down_kernel"
 *   fskhip_processor_process_ratecvt_*  "processor_io_ratecvt_kernel" or "processor_io_kernel+ratecvt_playback_kernel"; the
 *                                       _any_ forms "processor_io_ratecvt_kernel<any>" or
 *                                       "processor_io_kernel+ratecvt_playback_any_kernel", and the whole-period names where the
 *                                       quantum is whole periods of both rates from position 0
 * The string is static.  FSKHIP_PROC_RATECVT_PAIR in a ratecvt form's flags sends a TX side that would take the fused kernel
 * through the two launches instead, with the same results bit for bit: for measurements and tests; the other forms ignore it.
 */
#define FSKHIP_PROC_RATECVT_PAIR 4u
const char *fskhip_processor_last_tx_kernel(const fskhip_processor *p);

/*
 * A rate converter through remap, snapshot and restore (ABI 8, additions; FSKHIP_ABI_VERSION stays 8): the handle follows its
 * streams with the SAME map the engine, the processor, the resident XModem handles and the resamplers were carried with, so a
 * receiver bank at 44.1 kHz attaches and detaches receivers, checkpoints and moves between GPUs without a click.  The five calls
 * mirror fskhip_resampler_remap ... argument for argument, and the contract is theirs: remap and restore CREATE their handle, from
 * the source's or the image's own design (direction, up, down, taps as given to create, precision), so there is no destination that
 * could disagree; the device's tap order and table are made by create, never read from an image.  A converter's per-stream state is
 * its history row, fskhip_ratecvt_history() floats for fp32 and fp64 handles alike; the rows move on the device, by the resampler's
 * gather kernel.  Beside the rows a handle holds one word for all its streams, the position of the any-length calls, and it is
 * CARRIED: the new handle's position is the source's or the image's.  Synchronous host calls.
 *
 * fskhip_ratecvt_remap     *out: a new handle on src's device with src's design and position, for n_map streams.  Stream i
 *                          continues stream map[i] of src: its history row verbatim, every bit (NaN payloads and the sign of zero
 *                          included).  Where map[i] = -1 stream i starts with a zero row: at a position that is not 0 that is a
 *                          stream that has received zeros since the boundary, which is what fskhip_ratecvt_reset(r, stream) means
 *                          already.  A source named several times gives independent clones; sources not named are dropped.  src
 *                          is read only and stays usable.  Destroy *out with fskhip_ratecvt_destroy.
 * A rate converter snapshot is a host-side image: plain little-endian bytes, no pointers, every byte defined.  It is canonical: two
 * handles in the same observable state give the same bytes, whichever of their two history buffers is current.
 *   header, 64 bytes:  u32 magic "FSKC" (0x434B5346) | u32 format (1) | u32 header_bytes (64) | u32 record_bytes (4 x history) |
 *                      u32 n_records | u32 direction | u32 up | u32 down | u32 n_taps | u32 precision | u32 history | u32 position |
 *                      2 x u32 reserved (0) | u64 checksum
 *     history: ceil((n_taps - 1) / up).  checksum: the processor snapshot's function over the image's u64 words, with the checksum
 *     field taken as 0.
 *   the taps, n_taps doubles as given to create
 *   the rows, n_records x history floats packed tightly, one per selected stream, in selection order, oldest sample first
 *   zero padding to a multiple of 16 bytes
 * fskhip_ratecvt_snapshot_bytes  *bytes = the size of an image of n_sel records of this handle.
 * fskhip_ratecvt_snapshot        write streams[0 .. n_sel) (NULL: all streams, in order, whatever n_sel; a stream may be named more
 *                          than once) into image.  Synchronises with the device's outstanding work; the handle is read only and
 *                          stays usable.  *written (may be NULL) receives the size; cap too small (or image NULL):
 *                          FSKHIP_E_OVERFLOW with *written = the size needed and nothing written, so cap 0 is a size query.
 * fskhip_ratecvt_restore         remap with the image standing in for src, on any device: map[i] names a RECORD, or is -1; a NULL
 *                          map takes every record, in order (n_map is then ignored).  The design and the position are the image's.
 * fskhip_ratecvt_snapshot_info_get   what an image holds -- on the host, no device needed -- after validating ALL of it.
 *
 * Refusals, FSKHIP_E_INVALID before any device call, in this order; a refused call creates nothing, leaves *out alone and the
 * source as it was.
 *   remap           src or out NULL; map NULL with n_map > 0; n_map 0; the first map[i] below -1 or not below src's stream count.
 *   snapshot_bytes  r or bytes NULL.
 *   snapshot        r NULL; the first streams[i] below 0 or not below the handle's stream count; then the room (FSKHIP_E_OVERFLOW).
 *   an image        (info_get, restore) NULL; fewer bytes than a header; magic (a resampler's image is named as one); format;
 *                   header_bytes; a reserved word that is not 0; a direction that is neither; up, then down, outside 1..256; up and
 *                   down not coprime; n_taps outside 1..4096; a precision that is neither (create's limits); a history that is not
 *                   ceil((n_taps - 1) / up); a position not below down; record_bytes; the size against the layout above; the
 *                   checksum; a padding byte that is not zero.  info_get then: info NULL.
 *   restore         out NULL; the image; map non-NULL with n_map 0, or a NULL map over an image without records; the first map[i]
 *                   below -1 or not below the image's record count.  Then what create refuses for the device.
 */
typedef struct fskhip_ratecvt_snapshot_info {
  uint32_t n_streams;   /* records in the image */
  int direction;        /* FSKHIP_RATECVT_* */
  uint32_t up, down, n_taps;
  int precision;        /* FSKHIP_PRECISION_* */
  uint32_t history;     /* floats per record */
  uint32_t position;    /* inputs taken since the last period boundary, below down */
} fskhip_ratecvt_snapshot_info;
int fskhip_ratecvt_remap(const fskhip_ratecvt *src, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out);
int fskhip_ratecvt_snapshot_bytes(const fskhip_ratecvt *r, uint32_t n_sel, size_t *bytes);
int fskhip_ratecvt_snapshot(const fskhip_ratecvt *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written);
int fskhip_ratecvt_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out);
int fskhip_ratecvt_snapshot_info_get(const void *image, size_t bytes, fskhip_ratecvt_snapshot_info *info);

/* ---------------------------------------------------------------------------------------------------
 * IIR half of src/dsp/filters.ts: IIRFilter (8-106) batched over streams, + FilterFactory.createIIR* (325-344; the
 * designs themselves are fskhip_butterworth_* in fskhip.h).  Inside the demodulator the same filter lives as three
 * hard-wired biquads; this is the generic class: Direct Form I of any order <= 8.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fskhip_iir fskhip_iir;

/* new IIRFilter(b, a) (filters.ts:17-42) for n_streams independent streams sharing one coefficient set; histories start
 * at zero.  The constructor's three errors come back as FSKHIP_E_INVALID with the reference's messages ('Feedforward
 * coefficients (b) cannot be empty', 'Feedback coefficients (a) cannot be empty', 'First feedback coefficient (a[0])
 * cannot be zero'); coefficients are normalised by a[0] exactly as filters.ts:30-39 does (b[i] /= a0, a[i] /= a0 for
 * i >= 1).  More than 9 coefficients on either side: FSKHIP_E_UNSUPPORTED (the kernel keeps eight past inputs and outputs
 * in registers).  precision: FSKHIP_PRECISION_F64 evaluates output += b[i] * x[n-i], output -= a[i] * y[n-i] in doubles
 * in the reference's order, every product and sum rounded on its own (bit-identical results), FSKHIP_PRECISION_F32 the same
 * operations in floats (separate multiplies and adds: the library is built with -ffp-contract=off). */
int fskhip_iir_create(int device, const double *b, uint32_t nb, const double *a, uint32_t na, uint32_t n_streams,
                      int precision, fskhip_iir **out);
int fskhip_iir_destroy(fskhip_iir *f);
uint32_t fskhip_iir_streams(const fskhip_iir *f);   /* the n_streams it was created for (0 for NULL); ABI 7 */
/* getCoefficients() (filters.ts:103-105): the normalised sets; b and a must hold 9 doubles each. */
int fskhip_iir_get_coefficients(const fskhip_iir *f, double *b, uint32_t *nb, double *a, uint32_t *na);
/* processBuffer(input) (filters.ts:81-87) for every stream: out[s][t] = f32(process(in[s][t])), the histories carried
 * across calls.  in/out are [n_streams][pitch] float32; in == out (in place) is allowed. */
int fskhip_iir_process_device(fskhip_iir *f, const float *d_in, size_t n_per_stream, size_t in_pitch, float *d_out,
                              size_t out_pitch, void *hip_stream);
int fskhip_iir_process_host(fskhip_iir *f, const float *in, size_t n_per_stream, size_t in_pitch, float *out,
                            size_t out_pitch);
/* process(input) (filters.ts:47-76) sample by sample, numbers in and out (doubles, nothing rounded to float);
 * shares the histories with the Float32Array calls above. */
int fskhip_iir_process_f64_device(fskhip_iir *f, const double *d_in, size_t n_per_stream, size_t in_pitch, double *d_out,
                                  size_t out_pitch, void *hip_stream);
int fskhip_iir_process_f64_host(fskhip_iir *f, const double *in, size_t n_per_stream, size_t in_pitch, double *out,
                                size_t out_pitch);
/* reset() (filters.ts:92-98) for one stream, or all when stream < 0. */
int fskhip_iir_reset(fskhip_iir *f, int64_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FSKHIP_NEXT_H */
