// next_refusals_check.cpp -- the refusals of the filter and XModem host entry points that need no device, from a program of
// its own: for a sanitizer run of the library's HOST code on a machine without a GPU (tests/test_next_refusals_cpu.py holds the
// same calls to their exact texts through ctypes).  Build the C-ABI units with -Xarch_host -fsanitize=address,undefined, e.g.
//   cd webaudio_modem_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     *.hip ../../tests/cpp/next_refusals_check.cpp -o next_refusals_check && ./next_refusals_check
// Exit status 0 and "ok" when every call returned what it should; the sanitizers report on their own.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fskhip.h"
#include "../../include/fskhip_next.h"

static int failures = 0;
static void expect(int rc, int code, const char *text, int line) {
  if (rc == code && (!text || std::strcmp(fskhip_last_error(), text) == 0)) return;
  std::printf("line %d: rc %d \"%s\", expected %d \"%s\"\n", line, rc, fskhip_last_error(), code, text ? text : "(any)");
  failures++;
}
#define EXPECT(call, code, text) expect((call), (code), (text), __LINE__)

int main() {
  const int n_dev = fskhip_device_count();
  const int dev = n_dev;   // one past the last device; with no device every index is refused the same way
  char no_dev[96];
  if (n_dev == 0) std::snprintf(no_dev, sizeof(no_dev), "no HIP device available (the engine has no CPU fallback)");
  else std::snprintf(no_dev, sizeof(no_dev), "device %d out of range (%d devices)", dev, n_dev);

  std::vector<double> taps(4097, 0.25), ones(11, 1.0);
  double zero_a[2] = {0.0, 1.0};
  fskhip_fir *fir = nullptr;
  fskhip_iir *iir = nullptr;
  EXPECT(fskhip_fir_create(0, nullptr, 2, 1, FSKHIP_PRECISION_F64, &fir), FSKHIP_E_INVALID, "fskhip_fir_create: null/zero argument");
  EXPECT(fskhip_fir_create(0, taps.data(), 2, 0, FSKHIP_PRECISION_F64, &fir), FSKHIP_E_INVALID, "fskhip_fir_create: null/zero argument");
  EXPECT(fskhip_fir_create(0, taps.data(), 4097, 1, 7, &fir), FSKHIP_E_INVALID, "unknown precision 7");
  EXPECT(fskhip_fir_create(0, taps.data(), 4097, 1, FSKHIP_PRECISION_F32, &fir), FSKHIP_E_UNSUPPORTED, "4097 taps do not fit the LDS tile (max 4096)");
  EXPECT(fskhip_fir_create(dev, taps.data(), 4096, 3, FSKHIP_PRECISION_F64, &fir), FSKHIP_E_NO_DEVICE, no_dev);
  EXPECT(fskhip_iir_create(0, ones.data(), 2, ones.data(), 2, 0, FSKHIP_PRECISION_F64, &iir), FSKHIP_E_INVALID, "fskhip_iir_create: null/zero argument");
  EXPECT(fskhip_iir_create(0, nullptr, 2, nullptr, 0, 1, 7, &iir), FSKHIP_E_INVALID, "Feedforward coefficients (b) cannot be empty");
  EXPECT(fskhip_iir_create(0, ones.data(), 11, ones.data(), 0, 1, 7, &iir), FSKHIP_E_INVALID, "Feedback coefficients (a) cannot be empty");
  EXPECT(fskhip_iir_create(0, ones.data(), 11, zero_a, 2, 1, 7, &iir), FSKHIP_E_INVALID, "First feedback coefficient (a[0]) cannot be zero");
  EXPECT(fskhip_iir_create(0, ones.data(), 11, ones.data(), 2, 1, 7, &iir), FSKHIP_E_INVALID, "unknown precision 7");
  EXPECT(fskhip_iir_create(0, ones.data(), 11, ones.data(), 2, 1, FSKHIP_PRECISION_F64, &iir), FSKHIP_E_UNSUPPORTED,
         "IIR order 10: the batched kernel keeps up to 8 past inputs and outputs in registers");
  EXPECT(fskhip_iir_create(dev, ones.data(), 9, ones.data(), 9, 3, FSKHIP_PRECISION_F32, &iir), FSKHIP_E_NO_DEVICE, no_dev);

  uint8_t bytes[2 * 16] = {0}, out[2 * 16] = {0};
  uint16_t crc[2] = {0, 0};
  uint32_t lens[2] = {8, 9}, fit[2] = {7, 0}, seqs[2] = {1, 255}, seq0[2] = {1, 0}, out_lens[2] = {0, 0};
  fskhip_xmodem_result res[2];
  EXPECT(fskhip_crc16_host(-5, nullptr, 0, nullptr, 0, nullptr), FSKHIP_OK, nullptr);
  EXPECT(fskhip_crc16_host(0, bytes, 8, nullptr, 2, crc), FSKHIP_E_INVALID, "fskhip_crc16_host: null buffer");
  EXPECT(fskhip_crc16_host(0, bytes, 8, lens, 2, crc), FSKHIP_E_INVALID, "lens[1] = 9 exceeds pitch 8");
  EXPECT(fskhip_crc16_host(dev, bytes, 8, fit, 2, crc), FSKHIP_E_NO_DEVICE, no_dev);
  EXPECT(fskhip_xmodem_serialize_host(-5, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr), FSKHIP_OK, nullptr);
  EXPECT(fskhip_xmodem_serialize_host(0, bytes, 8, fit, seqs, 2, nullptr, 13, out_lens), FSKHIP_E_INVALID, "fskhip_xmodem_serialize_host: null buffer");
  EXPECT(fskhip_xmodem_serialize_host(0, bytes, 8, fit, seq0, 2, out, 13, out_lens), FSKHIP_E_INVALID, "Invalid sequence: 0. Must be 1-255.");
  EXPECT(fskhip_xmodem_serialize_host(0, bytes, 8, lens, seqs, 2, out, 16, out_lens), FSKHIP_E_INVALID, "lens[1] = 9 exceeds payload_pitch 8");
  EXPECT(fskhip_xmodem_serialize_host(0, bytes, 8, lens, seqs, 2, out, 13, out_lens), FSKHIP_E_OVERFLOW, "row 0 needs 14 bytes, slab holds 13");
  EXPECT(fskhip_xmodem_serialize_host(dev, bytes, 8, fit, seqs, 2, out, 13, out_lens), FSKHIP_E_NO_DEVICE, no_dev);
  EXPECT(fskhip_xmodem_scan_host(-5, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr), FSKHIP_OK, nullptr);
  EXPECT(fskhip_xmodem_scan_host(0, bytes, 8, lens, nullptr, 2, out, 16, res), FSKHIP_E_INVALID, "fskhip_xmodem_scan_host: null buffer");
  EXPECT(fskhip_xmodem_scan_host(0, bytes, 8, lens, seqs, 2, out, 16, res), FSKHIP_E_INVALID, "counts[1] = 9 exceeds pitch 8");
  EXPECT(fskhip_xmodem_scan_host(dev, bytes, 8, fit, seqs, 2, out, 16, res), FSKHIP_E_NO_DEVICE, no_dev);

  float x[4] = {0}, y[4] = {0};
  double xd[4] = {0}, yd[4] = {0};
  EXPECT(fskhip_fir_process_host(nullptr, x, 4, 4, y, 4), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_fir_process_device(nullptr, x, 4, 4, y, 4, nullptr), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_fir_reset(nullptr, -1), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_iir_process_host(nullptr, x, 4, 4, y, 4), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_iir_process_device(nullptr, x, 4, 4, y, 4, nullptr), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_iir_process_f64_host(nullptr, xd, 0, 0, yd, 0), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_iir_process_f64_device(nullptr, xd, 4, 4, yd, 4, nullptr), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_iir_reset(nullptr, 3), FSKHIP_E_INVALID, "null filter");
  EXPECT(fskhip_fir_destroy(nullptr), FSKHIP_OK, nullptr);
  EXPECT(fskhip_iir_destroy(nullptr), FSKHIP_OK, nullptr);

  std::vector<double> d(6, -7.0);   // an even numTaps writes numTaps + 1 low-pass / high-pass taps: room for 5, one to spare
  EXPECT(fskhip_sinc_lowpass(1000, 48000, 5, nullptr), FSKHIP_E_INVALID, "fskhip_sinc_lowpass: bad argument");
  EXPECT(fskhip_sinc_highpass(1000, 48000, 0, d.data()), FSKHIP_E_INVALID, "fskhip_sinc_highpass: bad argument");
  EXPECT(fskhip_sinc_bandpass(1750, 800, 48000, 0, d.data()), FSKHIP_E_INVALID, "fskhip_sinc_bandpass: bad argument");
  EXPECT(fskhip_sinc_lowpass(1000, 48000, 4, d.data()), 5, nullptr);
  EXPECT(fskhip_sinc_highpass(1000, 48000, 5, d.data()), 5, nullptr);
  EXPECT(fskhip_sinc_highpass(1000, 48000, 4, d.data()), 5, nullptr);
  EXPECT(fskhip_sinc_bandpass(1750, 800, 48000, 4, d.data()), 4, nullptr);
  if (d[5] != -7.0) { std::printf("a design wrote past its taps\n"); failures++; }

  std::printf(failures ? "%d refusals differ\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
