// fsk_launch.h -- the one declaration of every host-callable function a kernel file defines.  Included by the defining
// .hip file and by its callers (the C-ABI units), so that a signature cannot drift between them; and what the demodulator's
// launchers share: the call's arguments (DemodCall) and the form of a kernel file's instantiation table (KernelEntry).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fskhip_next.h"
#include "fsk_newstream.h"
#include "fsk_params.h"

namespace fsk {
// What a demodulate launch takes from its call: every launch_demod_* gets one of these, then its kernel family's own arguments,
// and says through `name` what fskhip_last_kernel reports for the kernel it chose.
struct DemodCall {
  bool writeback, append;   // write the AGC's output back into `samples`; the call has produced output already
  float *samples; size_t n, pitch;
  uint8_t *out; size_t out_pitch;
  uint32_t *out_counts, *eod_counts;
  hipStream_t stream;
  // samples [first, first + len) of the call as a launch of their own (head / whole tiles / tail): behind an earlier launch it appends
  DemodCall sub(size_t first, size_t len) const { return {writeback, append || first > 0, samples + first, len, pitch, out, out_pitch, out_counts, eod_counts, stream}; }
};
// One instantiation of a kernel family -- the typed kernel pointer and the name reported for it, both from one spelling of the
// template arguments (spell them as the name has them: "false, true").  Each kernel file lists its instantiations once, in tables
// of these beside the selector that indexes them; its LDS limit and its launcher both go through the table.
template <typename Fn>
struct KernelEntry { Fn fn; const char *name; };
#define FSK_K(K, ...) {&K<__VA_ARGS__>, "fsk::" #K "<" #__VA_ARGS__ ">"}
// the eight instantiations K<R, format, layout> of a kernel that reads or writes the capture formats, [format][layout] in the
// order of include/fskhip.h's enums
#define FSK_FORMAT_KERNELS(K, R)                                                                                                      \
  {{FSK_K(K, R, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, R, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_SAMPLE_MAJOR)},       \
   {FSK_K(K, R, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, R, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_SAMPLE_MAJOR)},       \
   {FSK_K(K, R, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, R, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)},   \
   {FSK_K(K, R, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, R, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)}}
template <typename Entry, size_t N>
hipError_t set_lds_limit(const Entry (&table)[N], size_t bytes) {   // every instantiation's limit of dynamic LDS
  for (const Entry &k : table) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// streams per workgroup of the four- and seven-wave kernels as an index: 64 / 32 / 16 / 8 -> 0..3, anything else counts as 64
inline uint32_t blk_lanes_index(uint32_t lanes) { return lanes == 32u ? 1u : lanes == 16u ? 2u : lanes == 8u ? 3u : 0u; }

// fsk_demod.hip: the generic kernel (fp64, wide / fractional rings, streams out of lock step)
hipError_t launch_demod(const DemodCall &c, const DemodParams &P, const DemodState &S, int precision, bool uniform_ds, bool split2, const char **name);
bool demod_fast_applicable(int precision, bool uniform_even, const DemodParams &P, const DemodState &S, const float *samples, size_t pitch);
size_t demod_split2_lds_bytes(const DemodParams &P);
hipError_t set_demod_split2_lds_limit(size_t lds_bytes);
hipError_t set_demod_lds_limit(size_t lds_bytes);
size_t demod_lds_bytes(const DemodParams &P);
// fsk_pipe.hip: free-running front / ZIR-corrected back kernels
hipError_t launch_demod_pipe(const DemodCall &c, const DemodParams &P, const DemodState &S, const char **name);
hipError_t launch_demod_fused(const DemodCall &c, const DemodParams &P, const DemodState &S, const char **name);
hipError_t launch_demod_tail(const DemodCall &c, const DemodParams &P, const DemodState &S, int parity0, const char **name);
size_t demod_pipe_lds_bytes(const DemodParams &P);
size_t demod_fused_lds_bytes(const DemodParams &P);
hipError_t set_pipe_lds_limit(size_t pipe_bytes);
// fsk_blk.hip: four waves per group, block-batched back wave
size_t demod_blk_lds_bytes(const DemodParams &P);
size_t demod_blk_lds_bytes(const DemodParams &P, uint32_t y_slots);
bool demod_blk_applicable(const DemodParams &P);
hipError_t set_blk_lds_limit(const DemodParams &P);
hipError_t launch_demod_blk(const DemodCall &c, const DemodParams &P, const DemodState &S, uint32_t resident_wgs, uint32_t slice_tiles, uint32_t y_slots,
                            uint32_t lanes, uint32_t medium, const char **name);
uint32_t demod_blk_lanes(uint32_t n_streams, int device);
void demod_blk_plan(const DemodParams &P, uint32_t groups, int device, uint32_t *y_slots, uint32_t *resident_wgs);
uint32_t demod_blk_slices(const DemodParams &P, const DemodState &S, size_t n, uint32_t resident_wgs, uint32_t slice_tiles, uint32_t *slice_tiles_out);
size_t demod_blk_queue_words(uint32_t groups);
// fsk_blk6.hip: seven waves per group, for batches that leave every workgroup a compute unit of its own
size_t demod_blk6_lds_bytes(const DemodParams &P, uint32_t y_slots);
uint32_t demod_blk6_y_slots(const DemodParams &P);
uint32_t demod_blk6_min_y_slots();
bool demod_blk6_applicable(const DemodParams &P);
size_t demod_blk6_max_samples();
hipError_t set_blk6_lds_limit(const DemodParams &P);
uint32_t demod_blk6_default_rolemap(uint32_t lanes, bool uniform);
hipError_t launch_demod_blk6(const DemodCall &c, const DemodParams &P, const DemodState &S, uint32_t lanes, uint32_t y_slots, uint32_t rolemap, const char **name);
// fsk_mod.hip: modulator, synthetic workloads, and the FSKProcessor quantum's bookkeeping / TX kernels
hipError_t launch_modulate(const ModParams &M, const double *coef, const uint8_t *payloads, const uint32_t *lens, size_t payload_pitch, float *out, size_t out_pitch,
                           uint32_t *out_lens, hipStream_t st);
hipError_t launch_synth(const ModParams &M, const double *coef, float *out, size_t n, size_t pitch, uint32_t payload_len, uint64_t seed, uint32_t lead_max, double amp_lo,
                        double amp_hi, hipStream_t st);
hipError_t launch_awgn(float *buf, size_t n, size_t pitch, uint32_t n_streams, double snr_db, uint64_t seed, double *sigma, hipStream_t st);
hipError_t launch_probe_read(const float *buf, size_t n, size_t pitch, uint32_t n_streams, float *sink, hipStream_t st);
uint8_t host_synth_payload_byte(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t i);
void host_synth_stream_params(uint64_t seed, uint32_t stream, uint32_t lead_max, double amp_lo, double amp_hi, uint32_t *lead, double *amp);
hipError_t launch_processor_io(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch, const uint32_t *demod_counts,
                               bool do_rx, float *out, size_t n_out, size_t out_pitch, bool clear_rx_on_complete, hipStream_t st);
// the same quantum with `out` in a capture format and layout (FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*, checked by the caller; out_pitch in
// elements): one launch, the kernel encodes behind its generator.  float32 stream-major is launch_processor_io.
hipError_t launch_processor_io_fmt(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch, const uint32_t *demod_counts,
                                   bool do_rx, void *out, int format, int layout, size_t n_out, size_t out_pitch, bool clear_rx_on_complete, hipStream_t st);
// the same quantum with `out` at a decimator's low rate (fskhip_processor_process_rate_*): n_out > 0 outputs per stream of the
// n_out * factor samples the generator makes, filtered as launch_resample_down does (d_taps in `precision`, histories
// [n_streams][n_taps - 1], d_hist_in read and d_hist_out written) and encoded, in one launch.  hipErrorInvalidValue where
// processor_rate_plan (fsk_processor_rate_plan.h) does not fuse the filter or the layout: the caller runs launch_processor_io and
// launch_resample_down.
hipError_t launch_processor_io_rate(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch, const uint32_t *demod_counts,
                                    bool do_rx, void *out, int format, int layout, size_t n_out, size_t out_pitch, bool clear_rx_on_complete, int precision,
                                    uint32_t factor, uint32_t n_taps, const void *d_taps, const float *d_hist_in, float *d_hist_out, hipStream_t st);
// the same quantum with `out` behind a playback converter (fskhip_processor_process_ratecvt_*): n_out > 0 outputs per stream from
// the handle's position pos < down, out of the n_high samples the generator makes: ratecvt_in_count_any(up, down, pos, n_out) of
// them or more, as long as they write n_out.  pos = 0 with n_out a multiple of `up` and n_high = n_out / up * down is the kernel's
// whole-period form, everything else its any-length form.  The samples are filtered as launch_ratecvt's playback direction does at
// that position (d_taps [K][up] in output order in `precision`, histories [n_streams][ceil((n_taps - 1) / up)], d_hist_in read and
// d_hist_out written) and encoded, in one launch.  hipErrorInvalidValue where processor_ratecvt_plan (fsk_processor_rate_plan.h)
// does not fuse the filter or the layout: the caller runs launch_processor_io and launch_ratecvt.
hipError_t launch_processor_io_ratecvt(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch,
                                       const uint32_t *demod_counts, bool do_rx, void *out, int format, int layout, size_t n_out, size_t out_pitch,
                                       bool clear_rx_on_complete, int precision, uint32_t up, uint32_t down, uint32_t pos, size_t n_high,
                                       uint32_t n_taps, const void *d_taps, const float *d_hist_in, float *d_hist_out, hipStream_t st);
hipError_t launch_processor_tx_start(const ModParams &M, const ProcState &T, const uint8_t *payloads, const uint32_t *lens, size_t payload_pitch, const uint8_t *mask,
                                     hipStream_t st);
hipError_t launch_processor_rx_drain(const ProcState &T, uint32_t n_streams, uint8_t *out, size_t out_pitch, uint32_t *counts, hipStream_t st);
hipError_t launch_processor_reset(const ProcState &T, uint32_t n_streams, int64_t stream, bool rx, bool tx, hipStream_t st);
// fsk_remap.hip: the state gather of fskhip_remap_streams
hipError_t launch_remap(int precision, const RemapArgs &A, const int64_t *d_map, const DemodState &D, const DemodState &S, hipStream_t st);
// fsk_snapshot.hip: stream snapshots -- [field][stream] state <-> stream-major records, transposed through LDS.
// pack: records [0, count) of d_out = streams d_sel[first ..] of S (d_sel null: first, first + 1, ...).
// unpack: stream i of D takes record d_map[i] - rec_first of d_in where that is in [0, rec_count), a new stream's state where
// d_map[i] = -1 and fresh_too; other streams are left alone (a restore runs it once per slab of records).
hipError_t launch_snap_pack(const SnapLayout &L, const DemodState &S, uint32_t n_src, const int64_t *d_sel, uint32_t first, uint32_t count, void *d_out,
                            hipStream_t st);
hipError_t launch_snap_unpack(int precision, const SnapLayout &L, const DemodState &D, uint32_t n_dst, const int64_t *d_map, uint32_t rec_first, uint32_t rec_count,
                              bool fresh_too, const NewStream &N, const void *d_in, hipStream_t st);
// fsk_samples.hip: the capture formats (FSKHIP_SAMPLES_*) and layouts (FSKHIP_LAYOUT_*).  sample_bytes: 0 = unknown format.
// check_sample_format: FSKHIP_OK, or the refusal of a format or layout that is none, with `who` in front, that every entry point taking the pair gives.
size_t sample_bytes(int format);
int check_sample_format(const char *who, int format, int layout);
// ingest: those -> float32 [stream][dst_pitch], exact.  The caller has checked the arguments (fskhip_ingest_device); nothing is
// launched for an empty batch.
hipError_t launch_ingest(const void *d_src, int format, int layout, uint32_t n_streams, size_t n, size_t src_pitch, float *d_dst, size_t dst_pitch, hipStream_t st);
// egress: float32 [stream][src_pitch] -> the same formats and layouts, narrowed (include/fskhip.h: the encoders).  d_lens (may
// be null): elements from d_lens[s] on are the format's silence.  The caller has checked the arguments (fskhip_egress_device); nothing
// is launched for an empty batch.
hipError_t launch_egress(const float *d_src, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, size_t n, int format, int layout, void *d_dst,
                         size_t dst_pitch, hipStream_t st);
// fsk_resample.hip: integer-factor rate conversion between a capture format at the low rate and float32 [stream][pitch] at the high
// rate (fskhip_resampler_*).  The caller has checked the arguments; nothing is launched for an empty batch; hipErrorInvalidValue
// where the batch is more workgroups than one launch takes.  precision selects the taps' type (float / double).  up: d_phase_taps is
// [factor][ceil(n_taps / factor)], phase p's taps c[p], c[p + factor], ...; the histories are [n_streams][ceil((n_taps - 1) / factor)].
// down: d_taps as given, n_out = outputs per stream (the call reads n_out * factor inputs), histories [n_streams][n_taps - 1]; d_lens
// (may be null): inputs from d_lens[s] on read as 0.0f.  Both read d_hist_in and write the history after the call to d_hist_out.
hipError_t launch_resample_up(int precision, const void *d_src, int format, int layout, uint32_t n_streams, size_t n_in, size_t src_pitch, float *d_dst,
                              size_t dst_pitch, uint32_t factor, uint32_t n_taps, const void *d_phase_taps, const float *d_hist_in, float *d_hist_out,
                              hipStream_t st);
hipError_t launch_resample_down(int precision, const float *d_src, size_t n_out, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, void *d_dst,
                                int format, int layout, size_t dst_pitch, uint32_t factor, uint32_t n_taps, const void *d_taps, const float *d_hist_in,
                                float *d_hist_out, hipStream_t st);
// fsk_ratecvt.hip: rate conversion by up / down (fskhip_ratecvt_*), one launch of either direction (FSKHIP_RATECVT_*).  CAPTURE reads
// d_src in the format and layout and writes float32 rows to d_dst, PLAYBACK the other way round with d_lens as launch_resample_down
// takes it; any n_in > 0 inputs per stream from the handle's position pos < down (fsk_ratecvt_plan.h): the call writes
// ratecvt_out_count_any(up, down, pos, n_in) per stream, possibly none, and always the next history; pos = 0 with n_in a multiple
// of `down` runs the whole-period kernels.  d_taps [ceil(n_taps / up)][up] in output order and d_table (fsk_ratecvt_plan.h),
// histories [n_streams][ceil((n_taps - 1) / up)].  The caller has checked the arguments; hipErrorInvalidValue where the batch is
// more workgroups than one launch takes.
hipError_t launch_ratecvt(int direction, int precision, const void *d_src, size_t src_pitch, const uint32_t *d_lens, void *d_dst, size_t dst_pitch, int format,
                          int layout, uint32_t n_streams, uint32_t pos, size_t n_in, uint32_t up, uint32_t down, uint32_t n_taps, const void *d_taps,
                          const uint32_t *d_table, const float *d_hist_in, float *d_hist_out, hipStream_t st);
// fsk_resample_remap.hip: a resampler's history rows (H floats at a pitch of H floats, both bases 16-byte aligned) gathered through
// a map (fskhip_resampler_remap / _snapshot / _restore).  Row i of d_dst (n_rows rows) takes row d_map[i] of d_src -- row
// ident0 + i where d_map is null --, zeros where the entry is -1.  from_image: d_src is a staging slab holding records
// [first, first + count) of an image; the launch writes only the rows whose record is among them, and the -1 rows where fresh_too.
// Nothing is launched where n_rows * H is 0; hipErrorInvalidValue where it is more workgroups than one launch takes.
hipError_t launch_resampler_hist_gather(float *d_dst, uint64_t n_rows, uint32_t H, const int64_t *d_map, int64_t ident0, const float *d_src, bool from_image,
                                        int64_t first, int64_t count, bool fresh_too, hipStream_t st);
// fsk_processor_remap.hip: FSKProcessor state (ProcState) between processors and stream-major records (ProcImage).
// gather: stream i of D continues stream d_map[i] of S, or starts as a created one where d_map[i] = -1.
// unpack: the same from the slab I of an image's records; streams whose record is in another slab are left alone, new ones are
// written where fresh_too (a restore runs it once per slab).  pack: records [0, I.count) of d_out, canonical.
// max_payload: *d_out = the longest pending payload among streams d_idx[0 .. n) (null: 0 .. n - 1; entries < 0 skipped).
hipError_t launch_processor_gather(const ProcState &D, uint32_t n_dst, const int64_t *d_map, const ProcState &S, hipStream_t st);
hipError_t launch_processor_unpack(const ProcState &D, uint32_t n_dst, const int64_t *d_map, const ProcImage &I, bool fresh_too, hipStream_t st);
hipError_t launch_processor_pack(const ProcState &S, const int64_t *d_sel, const ProcImage &I, void *d_out, hipStream_t st);
hipError_t launch_processor_max_payload(const ProcState &S, const int64_t *d_idx, uint32_t n, uint32_t *d_out, hipStream_t st);
// fsk_drain.hip: the compacted RX drain (fskhip_processor_rx_drain_sparse_*).  The caller has checked the arguments.
// size: count + scan -- d_pairs (drain_sparse_pair_words(n_streams) words of scratch) takes each workgroup's exclusive
// {stream, byte} position, d_totals {n_active, n_bytes, 1 if both fit the caps else 0}.
// pack: given those, and only where d_totals[2] is 1, writes the lists and the bytes and advances the selected rings.
// totals: the scan half on its own, for any list of n_pairs workgroup pairs (the resident XModem receiver reduces its own).
size_t drain_sparse_pair_words(uint32_t n_streams);
hipError_t launch_drain_totals(uint32_t *d_pairs, uint32_t n_pairs, uint32_t cap_streams, uint64_t cap_bytes, uint32_t *d_totals, hipStream_t st);
hipError_t launch_drain_sparse_size(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, uint32_t min_len, uint32_t cap_streams, uint64_t cap_bytes,
                                    uint32_t *d_pairs, uint32_t *d_totals, hipStream_t st);
hipError_t launch_drain_sparse_pack(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, uint32_t min_len, const uint32_t *d_pairs,
                                    const uint32_t *d_totals, uint32_t *d_streams, uint32_t *d_offsets, uint8_t *d_data, hipStream_t st);
// fsk_xmodem_rx.hip: the resident XModem receiver (fskhip_xmodem_rx_poll_*).  The caller has checked the arguments.
// XmRxState: the receiver's per-stream state.  XmRxScratch: per stream the poll's result R', the bytes to take out of the ring and
// two flag bits; xmodem_rx_pair_words(n_streams) words of workgroup pairs.
// scan: walks the selected rings, fills the scratch and nothing else, then the totals {n_events, n_bytes, 1 if both fit the caps}.
// commit: given those, and only where d_totals[2] is 1, writes the lists, the results and the payloads, advances the rings and
// updates the state.
struct XmRxState { uint32_t *expected, *packets, *dropped; };
struct XmRxScratch { fskhip_xmodem_result *res; uint32_t *removed, *flags, *pairs; };
size_t xmodem_rx_pair_words(uint32_t n_streams);
hipError_t launch_xmodem_rx_scan(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const XmRxState &X, const XmRxScratch &W, uint32_t cap_streams,
                                 uint64_t cap_bytes, uint32_t *d_totals, hipStream_t st);
hipError_t launch_xmodem_rx_commit(const ProcState &T, uint32_t n_streams, const XmRxState &X, const XmRxScratch &W, const uint32_t *d_totals, uint32_t *d_streams,
                                   fskhip_xmodem_result *d_results, uint32_t *d_offsets, uint8_t *d_data, hipStream_t st);
// fsk_xmodem_tx.hip: the resident XModem sender (fskhip_xmodem_tx_poll_*).  The caller has checked the arguments.
// XmTxState: the sender's per-stream words, each stream's file as [file_off, file_off + file_len) of the packed store, and the two
// settings.  XmTxScratch: per stream the poll's event and flag word; xmodem_tx_pair_words(n_streams) words of workgroup pairs; the
// staging slab [n_streams][slab_pitch] (rows 16-byte aligned, slab_pitch >= max_payload + 6) with its lengths and mask, in the
// form launch_processor_tx_start takes.
// step: decides every selected stream's transition into the scratch, clears tx_mask and nothing else, then the totals
// {n_events, 0, 1 if they fit cap_streams}.  commit: given those, and only where d_totals[2] is 1, writes the lists, builds the
// packets into the slab (tx_lens / tx_mask set for the streams that transmit), empties the rings that gave their reply and updates
// the words; the caller launches launch_processor_tx_start(M, T, slab, tx_lens, slab_pitch, tx_mask) behind it.
// repack: the files of the streams with keep[s] from one packed store into another (old_off -> new_off).
struct XmTxState {
  uint32_t *state, *sequence, *index, *n_fragments, *retries, *sent, *retransmitted, *file_off, *file_len;
  const uint8_t *store;
  uint32_t max_payload, max_retries;
};
struct XmTxScratch {
  fskhip_xmodem_tx_event *ev;
  uint32_t *flags, *pairs;
  uint8_t *slab; uint32_t slab_pitch;
  uint32_t *tx_lens; uint8_t *tx_mask;
};
size_t xmodem_tx_pair_words(uint32_t n_streams);
hipError_t launch_xmodem_tx_step(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const uint8_t *d_abort, const XmTxState &X, const XmTxScratch &W,
                                 uint32_t cap_streams, uint32_t *d_totals, hipStream_t st);
hipError_t launch_xmodem_tx_commit(const ProcState &T, uint32_t n_streams, const XmTxState &X, const XmTxScratch &W, const uint32_t *d_totals, uint32_t *d_streams,
                                   fskhip_xmodem_tx_event *d_events, hipStream_t st);
hipError_t launch_xmodem_tx_repack(const uint8_t *d_old_store, const uint32_t *d_old_off, const uint32_t *d_new_off, const uint32_t *d_lens, const uint8_t *d_keep,
                                   uint32_t n_streams, uint8_t *d_new_store, hipStream_t st);
// fsk_xmodem_recv.hip: the resident XModem file receiver (fskhip_xmodem_recv_poll_*).  The caller has checked the arguments.
// XmRecvState: the receiver's per-stream words, the file rows [n_streams][file_cap] and the two settings.  XmRecvScratch: per
// stream the poll's event, flag word, the bytes to take out of the ring and where the accepted payload starts among the live ring
// bytes; xmodem_recv_pair_words(n_streams) words of workgroup pairs; the staging slab [n_streams][slab_pitch] with its lengths
// and mask, in the form launch_processor_tx_start takes.
// step: decides every selected stream's transition into the scratch, clears tx_mask and nothing else, then the totals
// {n_events, 0, 1 if they fit cap_streams}.  commit: given those, and only where d_totals[2] is 1, writes the lists, appends the
// accepted payloads to the file rows, advances the rings, updates the words and puts the control bytes into the slab (tx_lens /
// tx_mask set for the streams that transmit); the caller launches launch_processor_tx_start(M, T, slab, tx_lens, slab_pitch,
// tx_mask) behind it.
// files: pack -- the file rows of streams d_sel[0 .. n_sel) into d_packed at d_offsets (n_sel + 1 entries); otherwise the other
// way, file_len set to each file's length.
struct XmRecvState {
  uint32_t *state, *expected, *retries, *file_len, *packets, *dropped, *sent;
  uint8_t *files;
  uint32_t file_cap, max_retries;
};
struct XmRecvScratch {
  fskhip_xmodem_recv_event *ev;
  uint32_t *flags, *removed, *span, *pairs;
  uint8_t *slab; uint32_t slab_pitch;
  uint32_t *tx_lens; uint8_t *tx_mask;
};
size_t xmodem_recv_pair_words(uint32_t n_streams);
hipError_t launch_xmodem_recv_step(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const uint8_t *d_timeout, const uint8_t *d_abort,
                                   const XmRecvState &X, const XmRecvScratch &W, uint32_t cap_streams, uint32_t *d_totals, hipStream_t st);
hipError_t launch_xmodem_recv_commit(const ProcState &T, uint32_t n_streams, const XmRecvState &X, const XmRecvScratch &W, const uint32_t *d_totals,
                                     uint32_t *d_streams, fskhip_xmodem_recv_event *d_events, hipStream_t st);
hipError_t launch_xmodem_recv_files(bool pack, const XmRecvState &X, const uint32_t *d_sel, const uint64_t *d_offsets, uint32_t n_sel, uint8_t *d_packed,
                                    hipStream_t st);
// fsk_xmodem_remap.hip: the three resident XModem handles carried through remap, snapshot and restore (fskhip_xmodem_*_remap /
// _snapshot / _restore).  The caller has checked the arguments.
// XmWords: a handle's per-stream word arrays in the order of its image record, and what a new stream holds in each.
// gather: stream i of D takes the words of stream d_map[i] of S -- or, where S is null, words [0, D.n) of record d_map[i] of d_table
// (record_words words per record) --, the fresh values where d_map[i] = -1.  pack: record r of d_table = the words of stream
// d_sel[r] of S (null: r), zeros behind them; flag7: word 7 is stored as 0 / 1 (the sender's has_file from its fragment count).
// XmSpan: one file's move, byte offsets into the two bases.  copy: every span, byte-exact, any length and alignment; max_len: the
// longest span (how many workgroups share one).
// recv_plan: the spans of a file receiver's remap -- row d_map[i] of the source (file_len bytes) to row i --, in d_bad[0] the first
// i whose file exceeds dst_cap (else 0xFFFFFFFF) and in d_bad[1] the longest carried file.  file_offsets: d_offsets[r] = the bytes of the files of streams d_sel[0 .. r)
// (null: 0 .. r), n + 1 entries; d_sums: xmodem_offsets_scratch_words(n) 64-bit words, of which the last two end as the total and
// the longest file.  recv_spans: with those, the spans of a
// snapshot -- row d_sel[r] to d_offsets[r] of the image's file area.
struct XmWords { uint32_t *a[8]; uint32_t fresh[8]; uint32_t n; };
struct XmSpan { uint64_t src, dst, len; };
hipError_t launch_xmodem_words_gather(const XmWords &D, uint32_t n_dst, const int64_t *d_map, const XmWords *S, const uint32_t *d_table, uint32_t record_words,
                                      hipStream_t st);
hipError_t launch_xmodem_words_pack(const XmWords &S, const int64_t *d_sel, uint32_t n, uint32_t record_words, bool flag7, uint32_t *d_table, hipStream_t st);
hipError_t launch_xmodem_span_copy(const uint8_t *d_src, uint8_t *d_dst, const XmSpan *d_spans, uint32_t n_spans, uint64_t max_len, hipStream_t st);
hipError_t launch_xmodem_recv_plan(const uint32_t *d_src_len, uint32_t src_cap, uint32_t dst_cap, const int64_t *d_map, uint32_t n_dst, XmSpan *d_spans,
                                   uint32_t *d_bad, hipStream_t st);
size_t xmodem_offsets_scratch_words(uint32_t n);
hipError_t launch_xmodem_file_offsets(const uint32_t *d_len, const int64_t *d_sel, uint32_t n, uint64_t *d_offsets, uint64_t *d_sums, hipStream_t st);
hipError_t launch_xmodem_recv_spans(const uint32_t *d_len, uint32_t cap, const int64_t *d_sel, uint32_t n, const uint64_t *d_offsets, XmSpan *d_spans,
                                    hipStream_t st);
// fsk_xmodem_timer.hip: the wait timers around the file receiver's and the sender's poll (fskhip_xmodem_*_poll_timed_*; the rule
// is fsk_xmodem_timer.h's).  The caller has checked the arguments.
// XmTimerState: per stream the two words (waited, mark), and as scratch of one timed poll the words before fire (old_waited;
// saved: the mark, with what fire found the stream to be above it), the ring's live bytes before the poll (held) and the flag
// byte the poll takes as its timeout mask (receiver) or abort mask (sender).
// fire: before the poll, d_state the handle's state words; d_abort (sender only, may be null) is OR-ed into the flag.
// arm: behind the poll's commit on the same stream, d_ev the poll's per-stream event scratch, d_totals the poll's totals: where
// d_totals[2] is 0 it puts back what fire changed.
struct XmTimerState {
  uint32_t *waited, *mark;
  uint32_t *old_waited, *saved, *held;
  uint8_t *flag;
  uint32_t timeout_samples;
};
hipError_t launch_xmodem_timer_fire(const XmTimerState &W, bool is_recv, const uint32_t *d_state, const ProcState &T, uint32_t n_streams, const uint8_t *d_mask,
                                    const uint8_t *d_abort, uint32_t elapsed, hipStream_t st);
hipError_t launch_xmodem_timer_arm_recv(const XmTimerState &W, const fskhip_xmodem_recv_event *d_ev, const ProcState &T, uint32_t n_streams,
                                        const uint32_t *d_totals, hipStream_t st);
hipError_t launch_xmodem_timer_arm_tx(const XmTimerState &W, const fskhip_xmodem_tx_event *d_ev, const ProcState &T, uint32_t n_streams,
                                      const uint32_t *d_totals, hipStream_t st);
// the timers through remap, snapshot and restore (fskhip_xmodem_timer_remap / _snapshot / _restore): one kernel, only the two words
// of a stream.  gather: stream i of D takes waited and mark of stream d_map[i] of S, 0 and 0 where d_map[i] = -1.  pack: record r
// of d_table (waited, mark interleaved, 8-byte aligned) = the words of stream d_sel[r] of S (null: r).  unpack: gather from such a
// table in the place of S, d_map[i] naming a record.  The caller has checked every entry against the source's count.
hipError_t launch_xmodem_timer_gather(const XmTimerState &D, const XmTimerState &S, const int64_t *d_map, uint32_t n_dst, hipStream_t st);
hipError_t launch_xmodem_timer_pack(const XmTimerState &S, const int64_t *d_sel, uint32_t n_sel, uint32_t *d_table, hipStream_t st);
hipError_t launch_xmodem_timer_unpack(const XmTimerState &D, const uint32_t *d_table, const int64_t *d_map, uint32_t n_dst, hipStream_t st);
}  // namespace fsk
