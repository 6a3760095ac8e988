// fsk_create.hip -- C ABI of libfskhip.so (include/fskhip.h): configure-time parameter derivation, creating and destroying an
// engine, and what a new engine takes over from an old one (fskhip_carry_over, the host half of fskhip_remap_streams and what it
// shares with fskhip_restore_streams).
#include <new>

#include "fsk_engine.h"
#include "fsk_launch.h"

using namespace fsk;

// filters.ts:180-192 (low-pass) and 200-212 (high-pass): the two designs differ in b only
static void ref_butter_lp_hp(bool high, double cutoff, double sr, double b[3], double a[3]) {
  double nyquist = sr / 2;
  double nc = cutoff / nyquist;
  double c = std::tan(M_PI * nc / 2);
  double c2 = c * c;
  double s2c = M_SQRT2 * c;
  double den = 1 + s2c + c2;
  if (high) { b[0] = 1 / den; b[1] = -2 / den; b[2] = 1 / den; }
  else { b[0] = c2 / den; b[1] = 2 * c2 / den; b[2] = c2 / den; }
  a[0] = 1; a[1] = (2 * c2 - 2) / den; a[2] = (1 - s2c + c2) / den;
}
static void ref_butter_lp(double cutoff, double sr, double b[3], double a[3]) { ref_butter_lp_hp(false, cutoff, sr, b, a); }
static void ref_butter_bp(double fc, double bwHz, double sr, double b[3], double a[3]) {  // filters.ts:221-234
  double omega = 2 * M_PI * fc / sr;
  double bw = 2 * M_PI * bwHz / sr;
  double c = std::tan(bw / 2);
  double d = 2 * std::cos(omega);
  double c2 = c * c;
  double den = 1 + c + c2;
  b[0] = c / den; b[1] = 0; b[2] = -c / den;
  a[0] = 1; a[1] = (-d * (1 + c2)) / den; a[2] = (1 - c + c2) / den;
}

static bool shared_fields_equal(const fskhip_config &a, const fskhip_config &b) {
  if (a.sampleRate != b.sampleRate || a.baudRate != b.baudRate) return false;
  if (a.preambleLen != b.preambleLen || a.sfdLen != b.sfdLen) return false;
  if (std::memcmp(a.preamblePattern, b.preamblePattern, sizeof(int32_t) * a.preambleLen)) return false;
  if (std::memcmp(a.sfdPattern, b.sfdPattern, sizeof(int32_t) * a.sfdLen)) return false;
  if (a.startBits != b.startBits || a.stopBits != b.stopBits || a.parity != b.parity) return false;
  if (a.syncThreshold != b.syncThreshold || (a.agcEnabled != 0) != (b.agcEnabled != 0)) return false;
  return true;
}

// Every fskhip_config field (fsk.ts:5-17): what stream i of a remap's destination and the source stream it continues must share.
static bool config_equal(const fskhip_config &a, const fskhip_config &b) {
  return shared_fields_equal(a, b) && a.markFrequency == b.markFrequency && a.spaceFrequency == b.spaceFrequency &&
         a.preFilterBandwidth == b.preFilterBandwidth && (a.adaptiveThreshold != 0) == (b.adaptiveThreshold != 0);
}
static const fskhip_config &stream_config(const fskhip_engine *e, size_t s) { return e->cfgs.size() == 1 ? e->cfgs[0] : e->cfgs[s]; }

// Everything the engine derives from its configuration -- the reference's calculateParameters / initializeDSP restated, in
// doubles and in its order of operations (the fp64 path's parity with the reference rests on these): e->P, e->M, the
// per-stream coefficient and NCO-increment tables, matched_zero, demod_ok / demod_why.  No HIP call.
static int derive_params(const fskhip_config *cfgs, uint32_t n_cfgs, fskhip_engine *e, std::vector<double> &coef, std::vector<uint64_t> &inc) {
  const fskhip_config &c0 = cfgs[0];
  const uint32_t n_streams = e->n_streams;
  const int precision = e->precision;
  // calculateParameters (fsk.ts:426-444), in doubles like the reference
  const double downsampleRate = c0.sampleRate / 2;
  e->spb = std::floor(c0.sampleRate / c0.baudRate);
  e->bpb = 8 + c0.startBits + c0.stopBits + (c0.parity != 0 ? 1 : 0);
  const double dsSPB = std::floor(downsampleRate / c0.baudRate);
  if (dsSPB < 1) return fail(FSKHIP_E_UNSUPPORTED, "downsampledSamplesPerBit < 1");

  // preambleSfdBits via addByteToPattern (fsk.ts:159-173)
  std::vector<int> pat;
  auto add_byte = [&](int byte) {
    for (int i = 0; i < c0.startBits; i++) pat.push_back(0);
    for (int i = 7; i >= 0; i--) pat.push_back((byte >> i) & 1);
    if (c0.parity != 0) {
      int par = 0;
      for (int i = 0; i < 8; i++) par ^= (byte >> i) & 1;
      pat.push_back(c0.parity == 1 ? par : 1 - par);
    }
    for (int i = 0; i < c0.stopBits; i++) pat.push_back(1);
  };
  for (int i = 0; i < c0.preambleLen; i++) add_byte(c0.preamblePattern[i]);
  for (int i = 0; i < c0.sfdLen; i++) add_byte(c0.sfdPattern[i]);
  const uint32_t n_bits = (uint32_t)pat.size();
  char why[256];
  auto refuse = [&]() { e->demod_ok = false; e->demod_why = why; };   // (after snprintf into `why`)
  if (n_bits > 63) { snprintf(why, sizeof(why), "%u preamble+SFD pattern bits (max 63)", n_bits); refuse(); }
  const double ring_cap = ((double)n_bits + 32) * dsSPB * 1.1;  // fsk.ts:145,149
  bool frac = false;
  if (e->demod_ok && ring_cap > 4.0e9) { snprintf(why, sizeof(why), "sync ring capacity %.17g too large", ring_cap); refuse(); }
  if (e->demod_ok && ring_cap != std::floor(ring_cap)) {
    // Fractional capacity: the reference's RingBuffer freezes after floor(cap) pushes (see
    // fsk_demod.hip).  That model holds while the index sequence w -> (w+1) % cap stays
    // non-integral: w = p - n*cap exactly (all values sit on cap's ulp grid), so it turns integral
    // again after n = 2^k/gcd(m,2^k) wraps where frac(cap) = m/2^k.  Refuse if that can happen
    // within 2^40 pushes.
    frac = true;
    double f = ring_cap - std::floor(ring_cap);
    int k = 0;
    while (f != std::floor(f) && k < 80) { f *= 2; k++; }
    // f is now the odd-or-even integer m scaled by 2^k; strip common factors of two
    double m = f;
    int v2 = 0;
    while (k - v2 > 0 && std::fmod(m, 2.0) == 0.0) { m /= 2; v2++; }
    const double wraps = std::ldexp(1.0, k - v2);
    if (wraps * std::floor(ring_cap) < 1.0995e12) {
      snprintf(why, sizeof(why),
               "sync ring capacity %.17g: the reference's fractional ring index turns integral again after "
               "%.0f wraps (fsk.ts:149, utils.ts:38-48); not emulated", ring_cap, wraps);
      refuse();
    }
  }
  DemodParams &P = e->P;
  P.n_streams = n_streams;
  P.d = (uint32_t)dsSPB;
  P.cadence = (uint32_t)std::floor(dsSPB / 4 + 0.5);  // Math.round
  P.n_bits = n_bits;
  P.sample_count = n_bits * P.d;
  P.frac = frac ? 1u : 0u;
  P.ring_int = e->demod_ok ? (uint32_t)std::floor(ring_cap) : 0u;
  // utils.ts:42-43: _length grows while < maxLength, so it saturates at floor(cap)+1 when fractional
  P.ring_cap = e->demod_ok ? (uint32_t)std::floor(ring_cap) + (frac ? 1u : 0u) : 0u;
  P.amp_cap = 8 * P.d;
  {
    const double total = (double)P.sample_count;
    P.matched_min = 0xFFFFFFFEu;  // never (0xFFFFFFFF is the kernels' "frame started" marker)
    if (P.sample_count > 0)
      for (uint32_t m = 0; m <= P.sample_count; m++)
        if ((double)m / total > c0.syncThreshold) { P.matched_min = m; break; }
  }
  {
    const double for_eod = e->bpb * dsSPB * 0.7;  // fsk.ts:148
    // sampleCount is >= 1 when the compare runs, so a threshold <= 1 behaves like 1
    double m = std::ceil(for_eod);
    P.eod_min = m <= 1 ? 1u : (uint32_t)m;
    // opt-in signal-quality estimates (include/fskhip.h)
    P.quality = 0;
    P.q_eod_n = (uint32_t)std::floor(for_eod);
    P.q_last_d0 = (uint32_t)((c0.sfdLen > 0 ? c0.sfdPattern[c0.sfdLen - 1] : c0.preambleLen > 0 ? c0.preamblePattern[c0.preambleLen - 1] : 1) & 1);
  }
  P.pat_q = 0; P.pat_mask = 0;
  for (uint32_t j = 1; j < n_bits && j < 64; j++) {
    P.pat_mask |= 1ull << j;
    if (pat[n_bits - j]) P.pat_q |= 1ull << j;
  }
  P.wide = (n_bits > 31 || frac) ? 1u : 0u;
  const uint32_t matched_zero = P.d * (uint32_t)__builtin_popcountll(~P.pat_q & P.pat_mask);
  e->matched_zero = matched_zero;
  P.stop_pos = c0.parity == 0 ? 9 : 10;  // fsk.ts:348
  P.parity_on = c0.parity != 0;
  P.agc_on = c0.agcEnabled != 0;
  {
    double b[3], a[3];
    ref_butter_lp(c0.baudRate, c0.sampleRate, b, a);  // fsk.ts:458-461
    P.lp_b0 = b[0]; P.lp_b1 = b[1]; P.lp_b2 = b[2]; P.lp_a1 = a[1]; P.lp_a2 = a[2];
  }
  P.agc_attack = 1.0 - std::exp(-1.0 / (c0.sampleRate * 0.001));  // fsk.ts:48-49
  P.agc_release = 1.0 - std::exp(-1.0 / (c0.sampleRate * 0.01));
  if (!P.agc_on) { P.agc_attack = 0.0; P.agc_release = 0.0; }  // fp32 kernels run the AGC block as a no-op
  P.f_lp_b0 = (float)P.lp_b0; P.f_lp_b0h = (float)(0.5 * P.lp_b0); P.f_lp_a2 = (float)P.lp_a2;
  // delta = 1 + a1 + a2 formed in f64, then rounded (see fsk_demod.hip lp32)
  P.f_lp_delta = (float)(1.0 + P.lp_a1 + P.lp_a2);
  P.f_agc_att = (float)P.agc_attack; P.f_agc_rel = (float)P.agc_release;

  ModParams &M = e->M;
  M.n_streams = n_streams;
  M.spb = (uint32_t)e->spb;
  M.bits_per_byte = (uint32_t)e->bpb;
  M.start_bits = c0.startBits; M.stop_bits = c0.stopBits; M.parity = c0.parity;
  M.exact_sin = precision == FSKHIP_PRECISION_F64 ? 1u : 0u;
  M.n_pre = c0.preambleLen + c0.sfdLen;
  for (int i = 0; i < c0.preambleLen; i++) M.pre[i] = (uint8_t)c0.preamblePattern[i];
  for (int i = 0; i < c0.sfdLen; i++) M.pre[c0.preambleLen + i] = (uint8_t)c0.sfdPattern[i];

  e->n_blocks = (n_streams + 63) / 64;
  e->lds_bytes = demod_lds_bytes(P);
  if (e->demod_ok && e->lds_bytes > 160 * 1024) { snprintf(why, sizeof(why), "dsSPB %u needs %zu B of LDS per wave (> 160 KiB)", P.d, e->lds_bytes); refuse(); }
  // per-stream constants (fsk.ts:451-456, 228, 404)
  coef.assign((size_t)CF_COUNT * n_streams, 0.0);
  inc.assign(n_streams, 0);
  for (uint32_t s = 0; s < n_streams; s++) {
    const fskhip_config &c = cfgs[n_cfgs == 1 ? 0 : s];
    const double center = (c.markFrequency + c.spaceFrequency) / 2;
    const double span = std::fabs(c.spaceFrequency - c.markFrequency);
    const double carson = 2 * (span / 2 + c.baudRate);
    const double bw = c.preFilterBandwidth > carson ? c.preFilterBandwidth : carson;
    double b[3], a[3];
    ref_butter_bp(center, bw, c.sampleRate, b, a);
    coef[(size_t)CF_bp_b0 * n_streams + s] = b[0];
    coef[(size_t)CF_bp_a1 * n_streams + s] = a[1];
    coef[(size_t)CF_bp_a2 * n_streams + s] = a[2];
    coef[(size_t)CF_omega * n_streams + s] = 2 * M_PI * center / c.sampleRate;
    coef[(size_t)CF_mark_w * n_streams + s] = 2 * M_PI * c.markFrequency / c.sampleRate;
    coef[(size_t)CF_space_w * n_streams + s] = 2 * M_PI * c.spaceFrequency / c.sampleRate;
    for (int k = 1; k <= 3; k++) {
      const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k * (long double)center /
                              (long double)c.sampleRate;
      coef[(size_t)(CF_w1_re + 2 * (k - 1)) * n_streams + s] = (double)cosl(ang);
      coef[(size_t)(CF_w1_im + 2 * (k - 1)) * n_streams + s] = (double)sinl(ang);
    }
    // NCO increment as a 64-bit fraction of a turn: frac(center/sr) * 2^64
    long double turns = (long double)center / (long double)c.sampleRate;
    turns -= std::floor(turns);
    long double scaled = turns * 18446744073709551616.0L;
    inc[s] = scaled >= 18446744073709551615.0L ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)(scaled + 0.5L);
  }

  P.uni_cfg = n_cfgs == 1 ? 1u : 0u;
  {
    const double b0 = coef[(size_t)CF_bp_b0 * n_streams], a1 = coef[(size_t)CF_bp_a1 * n_streams],
                 a2 = coef[(size_t)CF_bp_a2 * n_streams];
    P.u_bp_b0h = (float)(b0 * (0.5 * P.lp_b0));
    P.u_bp_na1 = (float)(-a1); P.u_bp_na2 = (float)(-a2);
    P.u_bp_c1y = (float)(a1 * a1 - a2); P.u_bp_c2y = (float)(a1 * a2);
    P.u_w1_re = (float)coef[(size_t)CF_w1_re * n_streams]; P.u_w1_im = (float)coef[(size_t)CF_w1_im * n_streams];
    P.u_w2_re = (float)coef[(size_t)CF_w2_re * n_streams]; P.u_w2_im = (float)coef[(size_t)CF_w2_im * n_streams];
    const uint64_t inc2 = inc[0] << 1, inc16 = inc[0] << 4;
    P.u_inc2_lo = (uint32_t)inc2; P.u_inc2_hi = (uint32_t)(inc2 >> 32);
    P.u_inc16_lo = (uint32_t)inc16; P.u_inc16_hi = (uint32_t)(inc16 >> 32);
    P.u_inc_lo = (uint32_t)inc[0]; P.u_inc_hi = (uint32_t)(inc[0] >> 32);
  }
  {
    // fsk_pipe.hip: zero-input response of the I/Q low-pass (y[n] = -a1 y[n-1] - a2 y[n-2]) as pair sums
    // q[m] = Z[2m] + Z[2m+1]:  q[m+2] = (a1^2 - 2 a2) q[m+1] - a2^2 q[m]  (the squared poles), and the map from the next
    // two pair sums back to the filter state (Z[n-1], Z[n-1] - Z[n-2]) at an even n (tools/zir_model.py)
    const double a1 = P.lp_a1, a2 = P.lp_a2;
    P.z_c1 = (float)(a1 * a1 - 2 * a2);
    P.z_c2 = (float)(a2 * a2);
    auto q_of = [&](double z1, double z2, double &q0, double &q1) {
      double Z[6] = {z2, z1, 0, 0, 0, 0};
      for (int i = 2; i < 6; i++) Z[i] = -a1 * Z[i - 1] - a2 * Z[i - 2];
      q0 = Z[2] + Z[3]; q1 = Z[4] + Z[5];
    };
    double l00, l10, l01, l11;           // q = L (zeta1, zeta2)
    q_of(1, 0, l00, l10);
    q_of(0, 1, l01, l11);
    const double det = l00 * l11 - l01 * l10;
    const double i00 = l11 / det, i01 = -l01 / det, i10 = -l10 / det, i11 = l00 / det;   // (zeta1, zeta2) = Linv (q0, q1)
    P.z_ya = (float)i00; P.z_yb = (float)i01;
    P.z_va = (float)(i00 - i10); P.z_vb = (float)(i01 - i11);
  }
  return FSKHIP_OK;
}

namespace {
// configure(): fresh FSKCore state for every stream (fsk.ts:101-131, 175-188; AGC gain 1.0 fsk.ts:46;
// silence.threshold 0.01 fsk.ts:128).  `matched` starts at its value for an all-zero bit history.
template <typename Real>
__global__ void init_kernel(DemodState S, uint32_t n, uint32_t matched_zero) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  Real *rs = (Real *)S.rs;
  for (int f = 0; f < RF_COUNT; f++) rs[(size_t)f * n + s] = (Real)0;
  for (int f = 0; f < IF_COUNT; f++) S.is[(size_t)f * n + s] = 0u;
  rs[(size_t)RF_agc_gain * n + s] = (Real)1.0;
  rs[(size_t)RF_nco_c * n + s] = (Real)1.0;       // (the fp64 NCO's phasor at phase 0)
  rs[(size_t)RF_sil_thr * n + s] = (Real)0.01;
  S.is[(size_t)IF_matched * n + s] = matched_zero;
  S.is[(size_t)IF_bit_wait * n + s] = kBigWait;
  S.is[(size_t)IF_zr_dph * n + s] = kHandPairs;
}
}  // namespace

// ---- what fskhip_remap_streams and fskhip_restore_streams (fsk_snapshot_api.hip) share: the checks, the lock-step decision and
// the host-side counters of a destination that continues streams of a StreamSource (fsk_engine.h)
namespace fsk {
bool config_shared_fields_equal(const fskhip_config &a, const fskhip_config &b) { return shared_fields_equal(a, b); }
bool config_all_fields_equal(const fskhip_config &a, const fskhip_config &b) { return config_equal(a, b); }
const fskhip_config &engine_stream_config(const fskhip_engine *e, size_t s) { return stream_config(e, s); }

int remap_check_map(const char *who, const char *what, const int64_t *map, uint32_t n_map) {
  if (n_map > 0 && !map) return fail(FSKHIP_E_INVALID, "%s: null map", who);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] < -1) return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld (%s or -1)", who, i, (long long)map[i], what);
  return FSKHIP_OK;
}

// a source that has reported (or now holds) a hand-off fault: its streams stopped mid-call.  Read only: e is not written.
// (After the caller's device synchronisation.)
int engine_refuse_handoff(const char *who, const char *the, const fskhip_engine *e) {
  uint32_t w = e->handoff_fault;
  if (w == 0u && e->S.blk_stat) HIP_TRY(hipMemcpy(&w, e->S.blk_stat + 2, sizeof(w), hipMemcpyDeviceToHost));
  if (w != 0u)
    return fail(FSKHIP_E_HANDOFF, "%s: %s's multi-wave kernel ran into its hand-off bound (fault word %u): its streams cannot be continued", who, the, w);
  return FSKHIP_OK;
}

int remap_check(const fskhip_engine *dst, const StreamSource &V, const int64_t *map, uint32_t n_map, RemapPlan *plan) {
  if (n_map != dst->n_streams) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", V.who, n_map, dst->n_streams);
  if (dst->precision != V.precision) return fail(FSKHIP_E_INVALID, "%s: engines differ in precision (%d, %d)", V.who, dst->precision, V.precision);
  if (dst->demodulated) return fail(FSKHIP_E_INVALID, "%s: the destination has demodulated already (remap into a fresh engine)", V.who);
  // One geometry for both engines, whatever the map (an all -1 map included): the gather reads src's state with dst's layout,
  // and dst takes over src's decimator phase and ring grid.  Every field but the per-stream tone pair / pre-filter bandwidth.
  if (!shared_fields_equal(dst->cfg0, V.cfg0) || dst->P.d != V.d || dst->P.amp_cap != V.amp_cap || dst->P.wide != V.wide ||
      dst->P.frac != V.frac || dst->P.n_bits != V.n_bits || dst->P.ring_cap != V.ring_cap)
    return fail(FSKHIP_E_INVALID, "%s: the engines' configurations differ beyond mark/space/preFilterBandwidth "
                "(sampleRate, baudRate, framing, patterns, syncThreshold, agcEnabled must be equal)", V.who);
  uint32_t n_fresh = 0;
  int64_t frame_row = -1;   // a continued stream's source row: its free-running I/Q frame is the one dst's continued streams share
  for (uint32_t i = 0; i < n_map; i++) {
    if (map[i] < 0) { n_fresh++; continue; }
    if (map[i] >= (int64_t)V.n_streams)
      return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, %s has %u %s", V.who, i, (long long)map[i], V.the, V.n_streams, V.unit);
    if (!config_equal(stream_config(dst, i), V.config(V.ctx, (size_t)map[i])))
      return fail(FSKHIP_E_INVALID, "%s: the config of stream %u differs from that of %s %lld", V.who, i, V.item, (long long)map[i]);
    if (frame_row < 0) frame_row = map[i];
  }
  // Lock step (one decimator phase, one ring grid for every stream) is what the whole-tile kernels need.  A continued stream
  // brings it along; a new one joins the grid -- unless the source streams are mid decimator-pair (a new one is not), the ring
  // capacity is fractional, or the source has left lock step already: then new streams start at the create-time positions and
  // the destination runs out of lock step, as after fskhip_reset of one stream mid-pair.
  plan->n_fresh = n_fresh;
  plan->frame_row = frame_row;
  plan->uniform = V.ds_uniform;
  plan->parity = V.ds_parity;
  plan->gen_odd = V.gen_odd;
  if (n_fresh == n_map) { plan->parity = 0; plan->gen_odd = false; }                 // only new streams: every decimator starts afresh
  else if (n_fresh > 0 && (V.ds_parity != 0 || V.frac)) plan->uniform = false;
  plan->grid = plan->uniform && !V.frac;
  // (fp32, one shared configuration in dst: new streams join the frame of a CONTINUED stream -- its config is dst's, unlike that of
  // an arbitrary source row of a per-stream source, whose NCO increment and therefore frame phase may be another)
  plan->frame = dst->precision == FSKHIP_PRECISION_F32 && dst->P.uni_cfg && frame_row >= 0;
  return FSKHIP_OK;
}

// host side: the engine's clocks and, per stream, the baselines its status counters are taken against (fsk.ts:131)
void remap_finish(fskhip_engine *dst, const StreamSource &V, const int64_t *map, uint32_t n_map, const RemapPlan &plan) {
  dst->calls = V.calls;
  dst->total_samples = V.total_samples;
  for (uint32_t i = 0; i < n_map; i++) {
    if (map[i] >= 0) V.baselines(V.ctx, (size_t)map[i], &dst->base_calls[i], &dst->base_samples[i]);
    else { dst->base_calls[i] = V.calls; dst->base_samples[i] = V.total_samples; }
  }
  dst->pushes = V.pushes;
  dst->ds_parity = plan.parity;
  dst->ds_uniform = plan.uniform;
  dst->gen_odd = plan.gen_odd;
  dst->P.quality = V.quality;   // the signal-quality estimates belong to the streams: they go on accumulating where they did
}
}  // namespace fsk

extern "C" {
void fskhip_butterworth_lowpass(double cutoff, double sr, double b[3], double a[3]) { ref_butter_lp(cutoff, sr, b, a); }
void fskhip_butterworth_highpass(double cutoff, double sr, double b[3], double a[3]) { ref_butter_lp_hp(true, cutoff, sr, b, a); }
void fskhip_butterworth_bandpass(double fc, double bw, double sr, double b[3], double a[3]) { ref_butter_bp(fc, bw, sr, b, a); }

void fskhip_default_config(fskhip_config *c) {  // fsk.ts:19-33
  std::memset(c, 0, sizeof(*c));
  c->sampleRate = 48000; c->baudRate = 1200; c->markFrequency = 1650; c->spaceFrequency = 1850;
  c->preamblePattern[0] = 0x55; c->preamblePattern[1] = 0x55; c->preambleLen = 2;
  c->sfdPattern[0] = 0x7E; c->sfdLen = 1;
  c->startBits = 1; c->stopBits = 1; c->parity = 0;
  c->syncThreshold = 0.85; c->agcEnabled = 1; c->preFilterBandwidth = 800; c->adaptiveThreshold = 1;
}
int fskhip_destroy(fskhip_engine *e) {
  if (!e) return FSKHIP_OK;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {e->S.rs, e->S.is, e->S.poly, e->S.amp_ring, (void *)e->S.coef, (void *)e->S.nco_inc, e->host.d_samples,
                  e->host.d_samples2, e->host.d_narrow[0], e->host.d_narrow[1], e->host.d_egress, e->host.d_out, e->host.d_counts, e->host.d_eod, e->host.d_lens, e->host.d_payloads, e->d_status, e->d_sigma,
                  e->S.trace_amp, e->S.trace_post, e->S.trace_bit, e->S.trace_n, e->S.poly_u, e->S.cu_ctr, e->S.blk_q, e->S.blk_stash, e->S.blk_stat, e->d_clock};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  if (e->blk.h_stat) (void)hipHostFree((void *)e->blk.h_stat);
  for (auto ev : e->timing.ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < 2; i++) {
    if (e->host.ev_copied[i]) (void)hipEventDestroy(e->host.ev_copied[i]);
    if (e->host.ev_used_up[i]) (void)hipEventDestroy(e->host.ev_used_up[i]);
  }
  if (e->host.copy_stream) (void)hipStreamDestroy(e->host.copy_stream);
  if (e->host.stream) (void)hipStreamDestroy(e->host.stream);
  delete e;
  return FSKHIP_OK;
}
int fskhip_create(const fskhip_config *cfgs, uint32_t n_cfgs, uint32_t n_streams, int device, int precision,
                  fskhip_engine **out) {
  if (!cfgs || !out || n_streams == 0) return fail(FSKHIP_E_INVALID, "fskhip_create: null/zero argument");
  if (n_cfgs != 1 && n_cfgs != n_streams) return fail(FSKHIP_E_INVALID, "n_cfgs must be 1 or n_streams");
  if (precision != FSKHIP_PRECISION_F32 && precision != FSKHIP_PRECISION_F64)
    return fail(FSKHIP_E_INVALID, "unknown precision %d", precision);
  const fskhip_config &c0 = cfgs[0];
  if (c0.preambleLen < 0 || c0.preambleLen > FSKHIP_MAX_PATTERN_BYTES || c0.sfdLen < 0 ||
      c0.sfdLen > FSKHIP_MAX_PATTERN_BYTES || c0.startBits < 0 || c0.stopBits < 0 || c0.startBits > 8 ||
      c0.stopBits > 8 || c0.parity < 0 || c0.parity > 2)
    return fail(FSKHIP_E_INVALID, "bad framing fields");
  if (!(c0.sampleRate > 0) || !(c0.baudRate > 0)) return fail(FSKHIP_E_INVALID, "sampleRate/baudRate must be > 0");
  for (uint32_t i = 1; i < n_cfgs; i++)
    if (!shared_fields_equal(c0, cfgs[i]))
      return fail(FSKHIP_E_UNSUPPORTED, "per-stream configs may differ only in mark/space/preFilterBandwidth (stream %u)", i);

  if (const int rc = select_device(device)) return rc;

  fskhip_engine *e = new (std::nothrow) fskhip_engine();
  if (!e) return fail(FSKHIP_E_NOMEM, "out of host memory");
  e->device = device; e->precision = precision; e->n_streams = n_streams; e->cfg0 = c0;
  e->cfgs.assign(cfgs, cfgs + n_cfgs);
  if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) e->cus = 0;
  e->split_cus = e->cus > 0 ? (uint32_t)e->cus : 256u;
  std::vector<double> coef;   // per-stream constants [CF_COUNT][n_streams]
  std::vector<uint64_t> inc;  // NCO increments [n_streams]
  if (const int rc = derive_params(cfgs, n_cfgs, e, coef, inc)) { delete e; return rc; }
  const DemodParams &P = e->P;

#define CREATE_TRY(expr) HIP_TRY_AS(expr, #expr, true, fskhip_destroy(e))
  const size_t rsz = precision == FSKHIP_PRECISION_F64 ? sizeof(double) : sizeof(float);
  CREATE_TRY(hipStreamCreateWithFlags(&e->host.stream, hipStreamNonBlocking));
  CREATE_TRY(hipMalloc(&e->S.rs, rsz * RF_COUNT * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.is, sizeof(uint32_t) * IF_COUNT * n_streams));
  const size_t poly_bytes = (P.wide ? sizeof(uint64_t) : sizeof(uint32_t)) * 64 * (size_t)P.d * e->n_blocks;
  CREATE_TRY(hipMalloc((void **)&e->S.poly, poly_bytes));
  CREATE_TRY(hipMalloc((void **)&e->S.amp_ring, sizeof(float) * (size_t)P.amp_cap * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.coef, sizeof(double) * coef.size()));
  CREATE_TRY(hipMalloc((void **)&e->S.nco_inc, sizeof(uint64_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_status, kStatusRawBytes));
  CREATE_TRY(hipMalloc((void **)&e->host.d_counts, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->host.d_eod, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->host.d_lens, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_sigma, sizeof(double) * n_streams));
  CREATE_TRY(hipMemcpy((void *)e->S.coef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice));
  CREATE_TRY(hipMemcpy((void *)e->S.nco_inc, inc.data(), sizeof(uint64_t) * n_streams, hipMemcpyHostToDevice));
  CREATE_TRY(hipMemset(e->S.poly, 0, poly_bytes));
  if (P.frac) {
    CREATE_TRY(hipMalloc((void **)&e->S.poly_u, poly_bytes));
    CREATE_TRY(hipMemset(e->S.poly_u, 0, poly_bytes));
  }
  CREATE_TRY(hipMemset(e->S.amp_ring, 0, sizeof(float) * (size_t)P.amp_cap * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.cu_ctr, sizeof(uint32_t) * 2048));
  CREATE_TRY(hipMemset(e->S.cu_ctr, 0, sizeof(uint32_t) * 2048));
  {
    dim3 g((n_streams + 255) / 256), b(256);
    if (precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(init_kernel<double>, g, b, 0, 0, e->S, n_streams, e->matched_zero);
    else hipLaunchKernelGGL(init_kernel<float>, g, b, 0, 0, e->S, n_streams, e->matched_zero);
    CREATE_TRY(hipGetLastError());
    CREATE_TRY(hipDeviceSynchronize());
  }
  if (e->demod_ok && e->lds_bytes > 48 * 1024) CREATE_TRY(set_demod_lds_limit(e->lds_bytes));
  if (e->demod_ok && precision == FSKHIP_PRECISION_F64 && !P.wide && !P.frac && demod_split2_lds_bytes(P) > 48 * 1024 && demod_split2_lds_bytes(P) <= 160 * 1024)
    CREATE_TRY(set_demod_split2_lds_limit(demod_split2_lds_bytes(P)));
  // {tiles, tiles off the fast loop, hand-off fault word, -}: the third word is every multi-wave kernel's (csrc/fsk_wait.h)
  CREATE_TRY(hipMalloc((void **)&e->S.blk_stat, 4 * sizeof(uint32_t)));
  CREATE_TRY(hipMemset(e->S.blk_stat, 0, 4 * sizeof(uint32_t)));
  e->M.stat = e->S.blk_stat;
  if (e->demod_ok && !P.wide && !P.frac && precision == FSKHIP_PRECISION_F32 && demod_pipe_lds_bytes(P) <= 160 * 1024)
    CREATE_TRY(set_pipe_lds_limit(demod_pipe_lds_bytes(P)));
  if (e->demod_ok && precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(P)) {
    CREATE_TRY(set_blk_lds_limit(P));
    CREATE_TRY(hipMalloc((void **)&e->S.blk_stash, sizeof(float) * 28u * (size_t)n_streams));
    CREATE_TRY(hipHostMalloc((void **)&e->blk.h_stat, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    e->blk.h_stat[0] = 0ull; e->blk.h_stat[1] = 0ull;
    e->blk.lanes = demod_blk_lanes(n_streams, device);
    demod_blk_plan(P, (n_streams + e->blk.lanes - 1u) / e->blk.lanes, device, &e->blk.y_slots, &e->blk.resident);
    if (demod_blk6_applicable(P)) CREATE_TRY(set_blk6_lds_limit(P));
    if (e->blk.resident && e->n_blocks > e->blk.resident) {
      CREATE_TRY(hipMalloc((void **)&e->S.blk_q, sizeof(uint32_t) * demod_blk_queue_words(e->n_blocks)));
    }
  }
  e->S.trace_stream = 0xFFFFFFFFu;
#undef CREATE_TRY
  e->base_calls.assign(n_streams, 0);
  e->base_samples.assign(n_streams, 0);
  *out = e;
  return FSKHIP_OK;
}
// What FSKCore.configure() on an already configured instance leaves in place (fsk.ts:133-157 rebuilds filters, rings and
// pattern and calls resetState(), 175-188): silence.threshold (fsk.ts:128, 321-326) and the debug counters (fsk.ts:131).
// A host re-configures by creating a new engine, carrying these over from the old one and destroying that.
int fskhip_carry_over(fskhip_engine *dst, const fskhip_engine *src) {
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "fskhip_carry_over: null engine");
  if (dst->n_streams != src->n_streams || dst->precision != src->precision || dst->device != src->device)
    return fail(FSKHIP_E_INVALID, "fskhip_carry_over: engines differ in stream count, precision or device");
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = dst->n_streams, at = engine_real_row(dst, RF_sil_thr);   // (equal stream counts and precision: one offset for both)
  HIP_TRY(hipMemcpy((char *)dst->S.rs + at, (const char *)src->S.rs + at, n * engine_real_bytes(dst), hipMemcpyDeviceToDevice));
  const int rows[] = {IF_sync_det, IF_eod_total};
  for (int f : rows)
    HIP_TRY(hipMemcpy(dst->S.is + (size_t)f * n, src->S.is + (size_t)f * n, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  dst->calls = src->calls;
  dst->total_samples = src->total_samples;
  dst->base_calls = src->base_calls;
  dst->base_samples = src->base_samples;
  return FSKHIP_OK;
}
// Stream i of dst continues stream map[i] of src as if that FSKCore had been moved, or (map[i] = -1) starts as a new one
// (include/fskhip.h).  Synchronous: every check first, then one gather launch (fsk_remap.hip), then the host-side counters.
int fskhip_remap_streams(fskhip_engine *dst, const fskhip_engine *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_remap_streams";
  if (const int rc = remap_check_map(who, "a source stream", map, n_map)) return rc;
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: null engine");
  if (dst == src) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: dst is src (remap into a new engine)");
  if (dst->device != src->device) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: engines are on devices %d and %d", dst->device, src->device);
  StreamSource V{};
  V.who = who; V.the = "the source"; V.unit = "streams"; V.item = "source stream";
  V.precision = src->precision; V.n_streams = src->n_streams; V.cfg0 = src->cfg0;
  V.d = src->P.d; V.amp_cap = src->P.amp_cap; V.wide = src->P.wide; V.frac = src->P.frac; V.n_bits = src->P.n_bits; V.ring_cap = src->P.ring_cap;
  V.calls = src->calls; V.total_samples = src->total_samples; V.pushes = src->pushes;
  V.ds_parity = src->ds_parity; V.ds_uniform = src->ds_uniform; V.gen_odd = src->gen_odd; V.quality = src->P.quality;
  V.ctx = src;
  V.config = [](const void *ctx, size_t s) { return stream_config((const fskhip_engine *)ctx, s); };
  V.baselines = [](const void *ctx, size_t s, uint64_t *calls, uint64_t *samples) {
    const fskhip_engine *e = (const fskhip_engine *)ctx;
    *calls = e->base_calls[s]; *samples = e->base_samples[s];
  };
  RemapPlan plan{};
  if (const int rc = remap_check(dst, V, map, n_map, &plan)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = engine_refuse_handoff(who, "the source", src)) return rc;

  RemapArgs A{};
  A.n_dst = dst->n_streams; A.n_src = src->n_streams;
  A.d = dst->P.d; A.amp_cap = dst->P.amp_cap; A.wide = dst->P.wide; A.frac = dst->P.frac;
  A.matched_zero = dst->matched_zero;
  A.grid_src = plan.grid ? 1u : 0u;
  A.frame_src = plan.frame ? 1u : 0u;
  A.frame_row = plan.frame_row >= 0 ? (uint32_t)plan.frame_row : 0u;
  int64_t *d_map = nullptr;
  HIP_TRY(hipMalloc((void **)&d_map, sizeof(int64_t) * n_map));
  hipError_t err = hipMemcpy(d_map, map, sizeof(int64_t) * n_map, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = launch_remap(dst->precision, A, d_map, dst->S, src->S, nullptr);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  (void)hipFree(d_map);
  if (err != hipSuccess) return fail(FSKHIP_E_HIP, "fskhip_remap_streams: %s", hipGetErrorString(err));
  remap_finish(dst, V, map, n_map, plan);
  return FSKHIP_OK;
}
}  // extern "C"
