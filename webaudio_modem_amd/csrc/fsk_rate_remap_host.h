// fsk_rate_remap_host.h -- remap, snapshot_bytes, snapshot and restore of the two rate converters' handles (fskhip_resampler:
// fsk_resample_remap_api.hip; fskhip_ratecvt: fsk_ratecvt_remap_api.hip), once, over their common base (RateHost,
// fsk_filter_host.h).  Each of remap and restore CREATES its handle, from the source's or the image's own taps, so there is no
// destination to mismatch.  The rows move on the device (fsk_resample_remap.hip: one gather kernel over a row length H and nothing
// else), into the new handle's hist[cur] only; an image's rows cross PCIe in slabs through fsk_stage.h's pipelines, its header,
// taps and padding being the host's.  An image is header | n_taps doubles | n_records rows of H floats | zeros to 16 bytes for both
// kinds; what differs is a kind's K:
//   Handle, Header, Image            the handle, the image's header and its validated view (fsk_*_image.h)
//   noun                             what the messages call a handle ("resampler")
//   magic, format, open              the image format's, and the one definition of a valid image
//   live_bytes, image_bytes          the format's layout functions (n_records, n_taps, history)
//   design(h, r)                     r's design and its words beside the rows (a position) into a header
//   create_like(src, n, out)         a handle of src's design and words for n streams, on src's device
//   create_from(device, h, taps, n, out)   the same from a validated image
//   destroy
// Not part of the ABI.
#pragma once
#include <cstring>
#include <vector>

#include "fsk_host.h"
#include "fsk_image.h"
#include "fsk_launch.h"
#include "fsk_stage.h"

namespace fsk {

// what remap and restore ask of a map over n_src rows (`noun`: "source" / "snapshot", `rows`: "streams" / "records"), in the
// header's order; a restore's null map (all records) has been replaced by the caller
inline int rate_check_map(const char *who, const char *kind, const int64_t *map, uint32_t n_map, const char *noun, const char *rows, uint32_t n_src) {
  if (!map && n_map > 0) return fail(FSKHIP_E_INVALID, "%s: null map with n_map %u", who, n_map);
  if (n_map == 0) return fail(FSKHIP_E_INVALID, "%s: n_map is 0: a %s has at least one stream", who, kind);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] < -1 || map[i] >= (int64_t)n_src)
      return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the %s has %u %s (-1: a new stream)", who, i, (long long)map[i], noun, n_src, rows);
  return FSKHIP_OK;
}

// a failed remap or restore leaves no handle
template <class K>
int rate_drop(typename K::Handle *r, int rc) {
  (void)hipDeviceSynchronize();
  (void)K::destroy(r);
  return rc;
}

template <class K>
int rate_remap(const char *who, const typename K::Handle *src, const int64_t *map, uint32_t n_map, typename K::Handle **out) {
  if (!src || !out) return fail(FSKHIP_E_INVALID, "%s: null %s", who, !src ? K::noun : "out");
  if (const int rc = rate_check_map(who, K::noun, map, n_map, "source", "streams", src->S)) return rc;
  HIP_TRY(hipSetDevice(src->device));
  HIP_TRY(hipDeviceSynchronize());
  typename K::Handle *r = nullptr;
  if (const int rc = K::create_like(src, n_map, &r)) return rc;
  if (r->H) {
    Scratch sc;
    int64_t *d_map = nullptr;
    if (const int rc = sc.upload(d_map, map, n_map)) return rate_drop<K>(r, rc);
    hipError_t err = launch_resampler_hist_gather(r->hist[r->cur], n_map, r->H, d_map, 0, src->hist[src->cur], false, 0, 0, false, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return rate_drop<K>(r, fail(FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err)));
  }
  *out = r;
  return FSKHIP_OK;
}

template <class K>
int rate_snapshot_bytes(const char *who, const typename K::Handle *r, uint32_t n_sel, size_t *bytes) {
  if (!r || !bytes) return fail(FSKHIP_E_INVALID, "%s: null %s", who, !r ? K::noun : "bytes");
  *bytes = (size_t)K::image_bytes(n_sel, r->n_taps, r->H);
  return FSKHIP_OK;
}

template <class K>
int rate_snapshot(const char *who, const typename K::Handle *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written) {
  using Header = typename K::Header;
  if (!r) return fail(FSKHIP_E_INVALID, "%s: null %s", who, K::noun);
  if (!streams) n_sel = r->S;
  if (const int rc = check_sel(who, K::noun, streams, n_sel, r->S)) return rc;
  const size_t rec_bytes = sizeof(float) * (size_t)r->H, need = (size_t)K::image_bytes(n_sel, r->n_taps, r->H);
  if (const int rc = check_room(who, n_sel, need, image, cap, written)) return rc;
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(hipDeviceSynchronize());

  Header h = image_header<Header>(K::magic, K::format);
  h.record_bytes = (uint32_t)rec_bytes; h.n_records = n_sel;
  K::design(h, r);
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
  const size_t live = (size_t)K::live_bytes(n_sel, r->n_taps, r->H);
  std::memset(out + live, 0, need - live);
  image_seal(h, out, need);
  return FSKHIP_OK;
}

template <class K>
int rate_restore(const char *who, int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, typename K::Handle **out) {
  if (!out) return fail(FSKHIP_E_INVALID, "%s: null out", who);
  typename K::Image im;
  if (const int rc = open_image(who, K::open, image, bytes, &im)) return rc;
  const typename K::Header &h = im.h;
  std::vector<int64_t> all;
  if (!map) {   // every record, in order
    all.resize(h.n_records);
    for (uint32_t i = 0; i < h.n_records; i++) all[i] = (int64_t)i;
    map = all.data(); n_map = h.n_records;
  }
  if (const int rc = rate_check_map(who, K::noun, map, n_map, "snapshot", "records", h.n_records)) return rc;
  std::vector<double> taps(h.n_taps);
  for (uint32_t i = 0; i < h.n_taps; i++) taps[i] = im.tap(i);
  typename K::Handle *r = nullptr;
  if (const int rc = K::create_from(device, h, taps.data(), n_map, &r)) return rc;
  if (r->H) {
    float *const rows = r->hist[r->cur];
    const uint32_t H = r->H;
    const auto unpack = [&](const int64_t *d_map, uint32_t first, uint32_t count, bool fresh_too, void *d_buf, hipStream_t stream) {
      return launch_resampler_hist_gather(rows, n_map, H, d_map, 0, (const float *)d_buf, true, (int64_t)first, (int64_t)count, fresh_too, stream);
    };
    if (const int rc = stage_records_in(who, r->stream, map, n_map, im.rows, h.n_records, h.record_bytes, unpack)) return rate_drop<K>(r, rc);
  }
  *out = r;
  return FSKHIP_OK;
}

}  // namespace fsk
