// rx_drain_sparse_check.cpp -- the refusals of fskhip_processor_rx_drain_sparse_host / _device that are made before any device
// call, from a program of its own: for a sanitizer run of the library's HOST code on a machine without a GPU
// (tests/test_rx_drain_sparse_cpu.py holds the same calls to their exact texts through ctypes).  Build the C-ABI units with
// -Xarch_host -fsanitize=address,undefined, e.g.
//   cd webaudio_modem_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     *.hip ../../tests/cpp/rx_drain_sparse_check.cpp -o rx_drain_sparse_check && ./rx_drain_sparse_check
// Exit status 0 and "ok" when every call returned what it should; the sanitizers report on their own.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/fskhip.h"
#include "../../include/fskhip_next.h"

static int failures = 0;
static void expect(int rc, int code, const char *text, int line) {
  if (rc == code && std::strcmp(fskhip_last_error(), text) == 0) return;
  std::printf("line %d: rc %d \"%s\", expected %d \"%s\"\n", line, rc, fskhip_last_error(), code, text);
  failures++;
}
#define EXPECT(call, code, text) expect((call), (code), (text), __LINE__)

int main() {
  uint32_t streams[4] = {9, 9, 9, 9}, offsets[5] = {9, 9, 9, 9, 9}, n_active = 7, n_bytes = 7, totals[3] = {7, 7, 7};
  uint8_t data[64] = {0}, mask[4] = {1, 0, 1, 1};
  const char *H = "fskhip_processor_rx_drain_sparse_host", *D = "fskhip_processor_rx_drain_sparse_device";
  char text[160];
  std::snprintf(text, sizeof(text), "%s: null n_active or n_bytes", H);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, streams, offsets, 4, data, 64, nullptr, &n_bytes), FSKHIP_E_INVALID, text);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, streams, offsets, 4, data, 64, &n_active, nullptr), FSKHIP_E_INVALID, text);
  std::snprintf(text, sizeof(text), "%s: null streams or offsets with cap_streams 4", H);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, nullptr, offsets, 4, data, 64, &n_active, &n_bytes), FSKHIP_E_INVALID, text);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, streams, nullptr, 4, data, 64, &n_active, &n_bytes), FSKHIP_E_INVALID, text);
  std::snprintf(text, sizeof(text), "%s: null data with cap_bytes 64", H);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, streams, offsets, 4, nullptr, 64, &n_active, &n_bytes), FSKHIP_E_INVALID, text);
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, mask, 1, streams, offsets, 4, data, 64, &n_active, &n_bytes), FSKHIP_E_INVALID, "null processor");
  EXPECT(fskhip_processor_rx_drain_sparse_host(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &n_active, &n_bytes), FSKHIP_E_INVALID, "null processor");
  std::snprintf(text, sizeof(text), "%s: null d_totals", D);
  EXPECT(fskhip_processor_rx_drain_sparse_device(nullptr, mask, 1, streams, offsets, 4, data, 64, nullptr, nullptr), FSKHIP_E_INVALID, text);
  std::snprintf(text, sizeof(text), "%s: null streams or offsets with cap_streams 2", D);
  EXPECT(fskhip_processor_rx_drain_sparse_device(nullptr, mask, 1, nullptr, nullptr, 2, data, 64, totals, nullptr), FSKHIP_E_INVALID, text);
  std::snprintf(text, sizeof(text), "%s: null data with cap_bytes 1", D);
  EXPECT(fskhip_processor_rx_drain_sparse_device(nullptr, mask, 1, streams, offsets, 2, nullptr, 1, totals, nullptr), FSKHIP_E_INVALID, text);
  EXPECT(fskhip_processor_rx_drain_sparse_device(nullptr, mask, 1, streams, offsets, 4, data, 64, totals, nullptr), FSKHIP_E_INVALID, "null processor");
  EXPECT(fskhip_processor_rx_drain_sparse_device(nullptr, nullptr, 9, nullptr, nullptr, 0, nullptr, 0, totals, nullptr), FSKHIP_E_INVALID, "null processor");
  // a refused call writes nothing
  if (n_active != 7 || n_bytes != 7 || totals[0] != 7 || totals[2] != 7 || streams[0] != 9 || offsets[4] != 9 || data[0] != 0) {
    std::printf("a refused call wrote to its outputs\n");
    failures++;
  }
  std::printf(failures ? "%d refusals differ\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
