// processor_image_concat_check.cpp -- the host-only concatenation of processor snapshots (csrc/fsk_processor_image.h:
// proc_image_concat, the definition behind fskhip_processor_snapshot_concat) as a stand-alone program, built with ASan + UBSan by
// tests/test_processor_sharded_cpu.py.  No kernel and no HIP is linked.  Images are written with the header's own writer helpers
// (proc_image_header, proc_image_bytes, image_seal) into heap blocks of exactly their size, at an odd address, so that a read or a
// write behind an image, or an aligned access, is caught.  1, 2 and 3 parts of 0, 1 and 65 records each, in every combination:
// record g of a case -- empty, wrapped and full rings, about a third of the records with a pending payload of ragged length -- is
// the same bytes whichever part holds it, each part has the payload capacity ITS records need, and the concatenation must be byte
// for byte the one image written for all the records; the size query must return that image's size; and each refusal must fire.
// stdout: "ok <cases> concatenations, <refusals> refusals"; a failure is named on stderr and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fsk_processor_image.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "line %d: ", __LINE__);         \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      failures++;                                          \
    }                                                      \
  } while (0)

// a heap block of exactly n bytes at an odd address
struct Block {
  unsigned char *base, *p;
  size_t n;
  explicit Block(size_t bytes) : base((unsigned char *)std::malloc(bytes + 1)), p(base + 1), n(bytes) { std::memset(p, 0xA5, n); }
  Block(const Block &) = delete;
  Block &operator=(const Block &) = delete;
  ~Block() { std::free(base); }
};

struct Rec {
  uint32_t w[12];
  double phase;
  std::vector<unsigned char> payload, ring;   // ring: rx_capacity bytes, canonical (zero outside the live span)
};

// record g of a case: a function of g (and the capacity) alone
Rec make_record(uint32_t g, uint32_t rx_cap) {
  Rec r;
  std::memset(r.w, 0, sizeof(r.w));
  r.phase = 0.0;
  r.ring.assign(rx_cap, 0);
  uint32_t read = 0, len = 0;
  switch (g % 4u) {
    case 0: break;                                                      // an empty ring
    case 1: read = rx_cap - 3u; len = 3u + (g % 7u); break;            // a wrapped one
    case 2: read = (g * 5u) % rx_cap; len = rx_cap; break;             // a full one
    default: read = g % rx_cap; len = 1u + (g % 5u); if (read + len > rx_cap) read = 0; break;
  }
  for (uint32_t i = 0; i < len; i++) r.ring[(read + i) % rx_cap] = (unsigned char)(1u + (g * 31u + i * 7u) % 255u);
  r.w[0] = (read + len) % rx_cap; r.w[1] = read; r.w[2] = len;
  r.w[4] = g % 3u;                                                      // completed
  if (g % 3u == 1u) {                                                   // a pending modulation of ragged length, mid-signal
    const uint32_t n = 1u + (g * 13u) % 40u;
    for (uint32_t i = 0; i < n; i++) r.payload.push_back((unsigned char)(g + i * 3u));
    r.w[3] = 1u; r.w[6] = 4800u + g; r.w[5] = (g * 97u) % r.w[6]; r.w[7] = n;
    r.w[8] = g % 40u; r.w[9] = g % 9u; r.w[10] = g & 1u;
    r.phase = 0.125 * (double)(g % 50u);
  }
  return r;
}

// the image of records [g0, g0 + n) of a case, as the library writes it: payload_capacity is what THESE records need
Block *write_image(uint32_t g0, uint32_t n, uint32_t rx_cap) {
  std::vector<Rec> recs;
  uint32_t max_pay = 0;
  for (uint32_t i = 0; i < n; i++) {
    recs.push_back(make_record(g0 + i, rx_cap));
    if (recs.back().payload.size() > max_pay) max_pay = (uint32_t)recs.back().payload.size();
  }
  const uint32_t pay_cap = (uint32_t)fsk::image_round16(max_pay);
  const fsk::ProcHeader h = fsk::proc_image_header(n, rx_cap, pay_cap);
  Block *b = new Block(fsk::proc_image_bytes(n, rx_cap, pay_cap));
  std::memset(b->p + sizeof(h), 0, b->n - sizeof(h));
  for (uint32_t i = 0; i < n; i++) {
    unsigned char *o = b->p + sizeof(h) + (size_t)i * h.record_bytes;
    std::memcpy(o, recs[i].w, 48);
    std::memcpy(o + 48, &recs[i].phase, 8);
    if (!recs[i].payload.empty()) std::memcpy(o + fsk::kProcRecFixed, recs[i].payload.data(), recs[i].payload.size());
    std::memcpy(o + fsk::kProcRecFixed + pay_cap, recs[i].ring.data(), rx_cap);
  }
  fsk::image_seal(h, b->p, b->n);
  return b;
}

struct Parts {
  std::vector<Block *> blocks;
  std::vector<const void *> bufs;
  std::vector<size_t> sizes;
  ~Parts() { for (Block *b : blocks) delete b; }
  void add(Block *b) { blocks.push_back(b); bufs.push_back(b->p); sizes.push_back(b->n); }
};

int concat(const Parts &P, void *out, size_t cap, size_t *written, std::string *text = nullptr) {
  char msg[512] = "";
  const int rc = fsk::proc_image_concat(P.bufs.data(), P.sizes.data(), (uint32_t)P.bufs.size(), out, cap, written, msg, sizeof(msg));
  if (text) *text = msg;
  return rc;
}

int cases = 0, refusals = 0;

void check_case(const std::vector<uint32_t> &counts, uint32_t rx_cap) {
  Parts P;
  uint32_t total = 0;
  for (uint32_t c : counts) { P.add(write_image(total, c, rx_cap)); total += c; }
  Block *whole = write_image(0, total, rx_cap);
  std::string name;
  for (uint32_t c : counts) name += std::to_string(c) + " ";
  name += "records, rx_capacity " + std::to_string(rx_cap);
  // every part and the whole are images the validator takes
  for (size_t k = 0; k < P.bufs.size(); k++) {
    fsk::ProcSnap s;
    char msg[512] = "";
    CHECK(fsk::proc_image_open(P.bufs[k], P.sizes[k], &s, msg, sizeof(msg)) == 0, "%s: part %zu is refused: %s", name.c_str(), k, msg);
  }
  size_t need = 0;
  std::string text;
  CHECK(concat(P, nullptr, 0, &need, &text) == fsk::kProcConcatOverflow, "%s: the size query does not return the overflow code (%s)", name.c_str(), text.c_str());
  CHECK(need == whole->n, "%s: the size query gives %zu, the image is %zu bytes", name.c_str(), need, whole->n);
  Block out(whole->n);
  size_t w = 0;
  const int rc = concat(P, out.p, out.n, &w, &text);
  CHECK(rc == 0, "%s: refused: %s", name.c_str(), text.c_str());
  CHECK(w == whole->n, "%s: written %zu of %zu", name.c_str(), w, whole->n);
  CHECK(rc == 0 && std::memcmp(out.p, whole->p, whole->n) == 0, "%s: the concatenation differs from the one image", name.c_str());
  // one byte short: refused, nothing written
  if (whole->n) {
    Block less(whole->n - 1);
    w = 0;
    CHECK(concat(P, less.p, less.n, &w, &text) == fsk::kProcConcatOverflow && w == whole->n, "%s: a buffer one byte short is not refused (%s)", name.c_str(), text.c_str());
    bool untouched = true;
    for (size_t i = 0; i < less.n; i++) untouched = untouched && less.p[i] == 0xA5;
    CHECK(untouched, "%s: a refused call wrote into the buffer", name.c_str());
    refusals++;
  }
  delete whole;
  cases++;
}

void expect_refusal(const char *what, const Parts &P, const char *pattern) {
  Block out(1 << 16);
  size_t w = 12345;
  std::string text;
  const int rc = concat(P, out.p, out.n, &w, &text);
  CHECK(rc == fsk::kProcConcatInvalid, "%s: returned %d (%s)", what, rc, text.c_str());
  CHECK(text.find(pattern) != std::string::npos, "%s: the message '%s' does not name '%s'", what, text.c_str(), pattern);
  bool untouched = true;
  for (size_t i = 0; i < out.n; i++) untouched = untouched && out.p[i] == 0xA5;
  CHECK(untouched, "%s: a refused call wrote into the buffer", what);
  refusals++;
}

}  // namespace

int main() {
  const uint32_t sizes[3] = {0u, 1u, 65u};
  for (uint32_t rx_cap : {48u, 50u}) {
    for (uint32_t a : sizes) {
      check_case({a}, rx_cap);
      for (uint32_t b : sizes) {
        check_case({a, b}, rx_cap);
        for (uint32_t c : sizes) check_case({a, b, c}, rx_cap);
      }
    }
  }
  {  // mixed rx_capacity
    Parts P;
    P.add(write_image(0, 3, 48)); P.add(write_image(3, 2, 64));
    expect_refusal("mixed rx_capacity", P, "differ in rx_capacity");
  }
  {  // a wrong stamp: another format's magic, and another format number, in the second part
    Parts P;
    P.add(write_image(0, 3, 48)); P.add(write_image(3, 2, 48));
    const uint32_t magic = 0x534B5346u;
    std::memcpy(P.blocks[1]->p, &magic, 4);
    expect_refusal("wrong magic", P, "magic");
    std::memcpy(P.blocks[1]->p, &fsk::kProcMagic, 4);
    const uint32_t format = 7;
    std::memcpy(P.blocks[1]->p + 4, &format, 4);
    expect_refusal("wrong format", P, "format 7");
  }
  {  // a truncated part
    Parts P;
    P.add(write_image(0, 65, 48)); P.add(write_image(65, 2, 48));
    P.sizes[0] -= 16;
    expect_refusal("truncated part", P, "do not match n_records x record_bytes");
    P.sizes[0] = 8;
    expect_refusal("part shorter than a header", P, "fewer than a processor snapshot header");
  }
  {  // one flipped checksum byte, and one flipped record byte
    Parts P;
    P.add(write_image(0, 2, 48)); P.add(write_image(2, 65, 48)); P.add(write_image(67, 1, 48));
    P.blocks[1]->p[offsetof(fsk::ProcHeader, checksum) + 3] ^= 0x10;
    expect_refusal("flipped checksum byte", P, "(snapshot 1)");
    expect_refusal("flipped checksum byte", P, "checksum");
    P.blocks[1]->p[offsetof(fsk::ProcHeader, checksum) + 3] ^= 0x10;
    P.blocks[2]->p[sizeof(fsk::ProcHeader) + fsk::kProcRecFixed + 5] ^= 0x01;
    expect_refusal("flipped ring byte", P, "(snapshot 2)");
  }
  {  // no parts, null arrays, a null part
    size_t w = 0;
    char msg[128] = "";
    Block out(64);
    CHECK(fsk::proc_image_concat(nullptr, nullptr, 0, out.p, out.n, &w, msg, sizeof(msg)) == fsk::kProcConcatInvalid, "no parts are not refused");
    Parts P;
    P.add(write_image(0, 1, 48));
    P.bufs[0] = nullptr;
    expect_refusal("null part", P, "null snapshot");
    refusals++;
  }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok %d concatenations, %d refusals\n", cases, refusals);
  return 0;
}
