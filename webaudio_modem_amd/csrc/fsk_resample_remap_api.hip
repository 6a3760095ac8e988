// fsk_resample_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): a resampler carried through the lifecycle calls the
// engine, the processor row and the resident XModem handles already have -- fskhip_resampler_remap, _snapshot_bytes, _snapshot,
// _restore and _snapshot_info_get.  The four calls that move rows are fsk_rate_remap_host.h's, which the rate converter shares
// (fsk_ratecvt_remap_api.hip); this file says what a resampler is to them: its image format and the one definition of a valid
// image (fsk_resample_image.h, host-only, on fsk_image.h's frame), its design and its create.  This file is the format's only writer.
#include "fsk_rate_remap_host.h"
#include "fsk_resample_image.h"
#include "fsk_resampler.h"

using namespace fsk;

namespace {

struct ResamplerKind {
  using Handle = fskhip_resampler;
  using Header = RsImageHeader;
  using Image = RsImage;
  static constexpr const char *noun = "resampler";
  static constexpr uint32_t magic = kRsMagic, format = kRsFormat;
  static int open(const void *buf, size_t size, Image *im, char *msg, size_t msg_cap) { return rs_image_open(buf, size, im, msg, msg_cap); }
  static uint64_t live_bytes(uint32_t n, uint32_t n_taps, uint32_t H) { return rs_live_bytes(n, n_taps, H); }
  static uint64_t image_bytes(uint32_t n, uint32_t n_taps, uint32_t H) { return rs_image_bytes(n, n_taps, H); }
  static void design(Header &h, const Handle *r) {
    h.direction = (uint32_t)r->direction; h.factor = r->L; h.n_taps = r->n_taps; h.precision = (uint32_t)r->precision; h.history = r->H;
  }
  static int create_like(const Handle *src, uint32_t n, Handle **out) {
    return fskhip_resampler_create(src->device, src->direction, src->L, src->h_taps.data(), src->n_taps, n, src->precision, out);
  }
  static int create_from(int device, const Header &h, const double *taps, uint32_t n, Handle **out) {
    return fskhip_resampler_create(device, (int)h.direction, h.factor, taps, h.n_taps, n, (int)h.precision, out);
  }
  static int destroy(Handle *r) { return fskhip_resampler_destroy(r); }
};

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
  return rate_remap<ResamplerKind>("fskhip_resampler_remap", src, map, n_map, out);
}

int fskhip_resampler_snapshot_bytes(const fskhip_resampler *r, uint32_t n_sel, size_t *bytes) {
  return rate_snapshot_bytes<ResamplerKind>("fskhip_resampler_snapshot_bytes", r, n_sel, bytes);
}

int fskhip_resampler_snapshot(const fskhip_resampler *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written) {
  return rate_snapshot<ResamplerKind>("fskhip_resampler_snapshot", r, streams, n_sel, image, cap, written);
}

int fskhip_resampler_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_resampler **out) {
  return rate_restore<ResamplerKind>("fskhip_resampler_restore", device, image, bytes, map, n_map, out);
}

}  // extern "C"
