// fsk_resample_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): a resampler carried through the lifecycle calls the
// engine, the processor row and the resident XModem handles already have -- fskhip_resampler_remap, _snapshot_bytes, _snapshot,
// _restore and _snapshot_info_get.  Each of remap and restore CREATES its handle (fskhip_resampler_create, from the source's or the
// image's own taps), so there is no destination to mismatch.  The rows move on the device (fsk_resample_remap.hip), into the new
// handle's hist[cur] only; an image's rows cross PCIe in slabs through fsk_stage.h's pipelines, its header, taps and padding
// being the host's.  The image's format and the one definition of a valid image are fsk_resample_image.h's (host-only, on
// fsk_image.h's frame); this file is the format's only writer.
#include <algorithm>

#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_resample_image.h"
#include "fsk_resampler.h"
#include "fsk_stage.h"

using namespace fsk;

namespace {

// what remap and restore ask of a map over n_src rows (`noun`: "source" / "snapshot", `rows`: "streams" / "records"), in the
// header's order; a restore's null map (all records) has been replaced by the caller
int check_map(const char *who, const int64_t *map, uint32_t n_map, const char *noun, const char *rows, uint32_t n_src) {
  if (!map && n_map > 0) return fail(FSKHIP_E_INVALID, "%s: null map with n_map %u", who, n_map);
  if (n_map == 0) return fail(FSKHIP_E_INVALID, "%s: n_map is 0: a resampler has at least one stream", who);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] < -1 || map[i] >= (int64_t)n_src)
      return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the %s has %u %s (-1: a new stream)", who, i, (long long)map[i], noun, n_src, rows);
  return FSKHIP_OK;
}

// a failed remap or restore leaves no handle
int drop(fskhip_resampler *r, int rc) {
  (void)hipDeviceSynchronize();
  (void)fskhip_resampler_destroy(r);
  return rc;
}

}  // namespace

extern "C" {

int fskhip_resampler_snapshot_info_get(const void *image, size_t bytes, fskhip_resampler_snapshot_info *info) {
  static const char who[] = "fskhip_resampler_snapshot_info_get";
  RsImage im;
  if (const int rc = open_image(who, rs_image_open, image, bytes, &im)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->n_streams = im.h.n_records; info->direction = (int)im.h.direction; info->factor = im.h.factor; info->n_taps = im.h.n_taps;
  info->precision = (int)im.h.precision; info->history = im.h.history;
  return FSKHIP_OK;
}

int fskhip_resampler_remap(const fskhip_resampler *src, const int64_t *map, uint32_t n_map, fskhip_resampler **out) {
  static const char who[] = "fskhip_resampler_remap";
  if (!src || !out) return fail(FSKHIP_E_INVALID, "%s: null %s", who, !src ? "resampler" : "out");
  if (const int rc = check_map(who, map, n_map, "source", "streams", src->S)) return rc;
  HIP_TRY(hipSetDevice(src->device));
  HIP_TRY(hipDeviceSynchronize());
  fskhip_resampler *r = nullptr;
  if (const int rc = fskhip_resampler_create(src->device, src->direction, src->L, src->h_taps.data(), src->n_taps, n_map, src->precision, &r)) return rc;
  if (r->H) {
    Scratch sc;
    int64_t *d_map = nullptr;
    if (const int rc = sc.upload(d_map, map, n_map)) return drop(r, rc);
    hipError_t err = launch_resampler_hist_gather(r->hist[r->cur], n_map, r->H, d_map, 0, src->hist[src->cur], false, 0, 0, false, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return drop(r, fail(FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err)));
  }
  *out = r;
  return FSKHIP_OK;
}

int fskhip_resampler_snapshot_bytes(const fskhip_resampler *r, uint32_t n_sel, size_t *bytes) {
  static const char who[] = "fskhip_resampler_snapshot_bytes";
  if (!r || !bytes) return fail(FSKHIP_E_INVALID, "%s: null %s", who, !r ? "resampler" : "bytes");
  *bytes = (size_t)rs_image_bytes(n_sel, r->n_taps, r->H);
  return FSKHIP_OK;
}

int fskhip_resampler_snapshot(const fskhip_resampler *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written) {
  static const char who[] = "fskhip_resampler_snapshot";
  if (!r) return fail(FSKHIP_E_INVALID, "%s: null resampler", who);
  if (!streams) n_sel = r->S;
  if (const int rc = check_sel(who, "resampler", streams, n_sel, r->S)) return rc;
  const size_t rec_bytes = sizeof(float) * (size_t)r->H, need = (size_t)rs_image_bytes(n_sel, r->n_taps, r->H);
  if (const int rc = check_room(who, n_sel, need, image, cap, written)) return rc;
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(hipDeviceSynchronize());

  RsImageHeader h = image_header<RsImageHeader>(kRsMagic, kRsFormat);
  h.record_bytes = (uint32_t)rec_bytes; h.n_records = n_sel;
  h.direction = (uint32_t)r->direction; h.factor = r->L; h.n_taps = r->n_taps; h.precision = (uint32_t)r->precision; h.history = r->H;
  unsigned char *out = (unsigned char *)image, *taps = out + sizeof(h), *rec = taps + sizeof(double) * (size_t)r->n_taps;
  if (rec_bytes && n_sel) {
    const float *rows = r->hist[r->cur];   // (the one buffer the next call reads: an image does not tell which of the two it was)
    const uint32_t H = r->H;
    const auto pack = [&](const int64_t *d_sel, uint32_t first, uint32_t count, void *d_buf, hipStream_t stream) {
      return launch_resampler_hist_gather((float *)d_buf, count, H, d_sel ? d_sel + first : nullptr, (int64_t)first, rows, false, 0, 0, false, stream);
    };
    const auto finish = [](uint32_t, uint32_t) {};   // (the checksum runs over taps, rows and padding at the end)
    if (const int rc = stage_records_out(who, r->stream, streams, n_sel, rec_bytes, rec, pack, finish)) return rc;
  }
  std::memcpy(taps, r->h_taps.data(), sizeof(double) * (size_t)r->n_taps);
  const size_t live = (size_t)rs_live_bytes(n_sel, r->n_taps, r->H);
  std::memset(out + live, 0, need - live);
  image_seal(h, out, need);
  return FSKHIP_OK;
}

int fskhip_resampler_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_resampler **out) {
  static const char who[] = "fskhip_resampler_restore";
  if (!out) return fail(FSKHIP_E_INVALID, "%s: null out", who);
  RsImage im;
  if (const int rc = open_image(who, rs_image_open, image, bytes, &im)) return rc;
  const RsImageHeader &h = im.h;
  std::vector<int64_t> all;
  if (!map) {   // every record, in order
    all.resize(h.n_records);
    for (uint32_t i = 0; i < h.n_records; i++) all[i] = (int64_t)i;
    map = all.data(); n_map = h.n_records;
  }
  if (const int rc = check_map(who, map, n_map, "snapshot", "records", h.n_records)) return rc;
  std::vector<double> taps(h.n_taps);
  for (uint32_t i = 0; i < h.n_taps; i++) taps[i] = im.tap(i);
  fskhip_resampler *r = nullptr;
  if (const int rc = fskhip_resampler_create(device, (int)h.direction, h.factor, taps.data(), h.n_taps, n_map, (int)h.precision, &r)) return rc;
  if (r->H) {
    float *const rows = r->hist[r->cur];
    const uint32_t H = r->H;
    const auto unpack = [&](const int64_t *d_map, uint32_t first, uint32_t count, bool fresh_too, void *d_buf, hipStream_t stream) {
      return launch_resampler_hist_gather(rows, n_map, H, d_map, 0, (const float *)d_buf, true, (int64_t)first, (int64_t)count, fresh_too, stream);
    };
    if (const int rc = stage_records_in(who, r->stream, map, n_map, im.rows, h.n_records, h.record_bytes, unpack)) return drop(r, rc);
  }
  *out = r;
  return FSKHIP_OK;
}

}  // extern "C"
