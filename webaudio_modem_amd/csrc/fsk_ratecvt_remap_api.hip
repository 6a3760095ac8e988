// fsk_ratecvt_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): a rate converter carried through the lifecycle calls
// the resampler has -- fskhip_ratecvt_remap, _snapshot_bytes, _snapshot, _restore and _snapshot_info_get.  The four calls that move
// rows are fsk_rate_remap_host.h's, shared with the resampler (fsk_resample_remap_api.hip), and so is the device half
// (fsk_resample_remap.hip: a converter's row is H = ceil((n_taps - 1) / up) <= 4 095 floats at a pitch of H, which is all that
// kernel knows of a row); this file says what a converter is to them: its image format and the one definition of a valid image
// (fsk_ratecvt_image.h, host-only, on fsk_image.h's frame), its design, its create, and the one word beside the rows -- the
// position, which the new handle takes from the source or the image.  The device's tap order and table are create's, never an
// image's.  This file is the format's only writer.
#include "fsk_rate_remap_host.h"
#include "fsk_ratecvt.h"
#include "fsk_ratecvt_image.h"

using namespace fsk;

namespace {

struct RatecvtKind {
  using Handle = fskhip_ratecvt;
  using Header = RcImageHeader;
  using Image = RcImage;
  static constexpr const char *noun = "rate converter";
  static constexpr uint32_t magic = kRcMagic, format = kRcFormat;
  static int open(const void *buf, size_t size, Image *im, char *msg, size_t msg_cap) { return rc_image_open(buf, size, im, msg, msg_cap); }
  static uint64_t live_bytes(uint32_t n, uint32_t n_taps, uint32_t H) { return rc_live_bytes(n, n_taps, H); }
  static uint64_t image_bytes(uint32_t n, uint32_t n_taps, uint32_t H) { return rc_image_bytes(n, n_taps, H); }
  static void design(Header &h, const Handle *r) {
    h.direction = (uint32_t)r->direction; h.up = r->L; h.down = r->M; h.n_taps = r->n_taps; h.precision = (uint32_t)r->precision; h.history = r->H;
    h.position = r->pos;
  }
  static int create_like(const Handle *src, uint32_t n, Handle **out) {
    if (const int rc = fskhip_ratecvt_create(src->device, src->direction, src->L, src->M, src->h_taps.data(), src->n_taps, n, src->precision, out)) return rc;
    (*out)->pos = src->pos;
    return FSKHIP_OK;
  }
  static int create_from(int device, const Header &h, const double *taps, uint32_t n, Handle **out) {
    if (const int rc = fskhip_ratecvt_create(device, (int)h.direction, h.up, h.down, taps, h.n_taps, n, (int)h.precision, out)) return rc;
    (*out)->pos = h.position;   // (rc_image_open has held it below `down`)
    return FSKHIP_OK;
  }
  static int destroy(Handle *r) { return fskhip_ratecvt_destroy(r); }
};

}  // namespace

extern "C" {

int fskhip_ratecvt_snapshot_info_get(const void *image, size_t bytes, fskhip_ratecvt_snapshot_info *info) {
  static const char who[] = "fskhip_ratecvt_snapshot_info_get";
  RcImage im;
  if (const int rc = open_image(who, rc_image_open, image, bytes, &im)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->n_streams = im.h.n_records; info->direction = (int)im.h.direction; info->up = im.h.up; info->down = im.h.down; info->n_taps = im.h.n_taps;
  info->precision = (int)im.h.precision; info->history = im.h.history; info->position = im.h.position;
  return FSKHIP_OK;
}

int fskhip_ratecvt_remap(const fskhip_ratecvt *src, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out) {
  return rate_remap<RatecvtKind>("fskhip_ratecvt_remap", src, map, n_map, out);
}

int fskhip_ratecvt_snapshot_bytes(const fskhip_ratecvt *r, uint32_t n_sel, size_t *bytes) {
  return rate_snapshot_bytes<RatecvtKind>("fskhip_ratecvt_snapshot_bytes", r, n_sel, bytes);
}

int fskhip_ratecvt_snapshot(const fskhip_ratecvt *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written) {
  return rate_snapshot<RatecvtKind>("fskhip_ratecvt_snapshot", r, streams, n_sel, image, cap, written);
}

int fskhip_ratecvt_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out) {
  return rate_restore<RatecvtKind>("fskhip_ratecvt_restore", device, image, bytes, map, n_map, out);
}

}  // extern "C"
