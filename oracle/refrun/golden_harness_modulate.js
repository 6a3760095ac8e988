// Golden-vector harness for the MODULATOR's untested configurations (TEST INFRASTRUCTURE, build container only).
//
// What the REAL reference FSKCore.modulateData (fsk.ts:377-424; type-stripped into a temp dir by strip_ts.py, never committed)
// writes at the samples-per-bit values on both sides of the library's 32-sample tile -- 5, 10, 20, 31 | 32, 33, 40, 64, 147 --
// crossed with the framings (8N1; even parity + two stop bits; odd parity + two start bits; no preamble and no SFD; a 4-byte
// preamble) and payloads of 0, 1 and 7 bytes; and long signals, one per side, whose phase passes the end of the medium range of
// fdlibm's sine (Cody-Waite reduction; Payne-Hanek beyond it) -- as its comment states it and as its code has it (LIMITS below).
//
// usage: node golden_harness_modulate.js <ref_bundle.js> <out_dir>     (make_golden.py drives it)
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const H = require('./golden_harness.js');
const { R, manifest, arrays, saveArray, rng32, mkCore } = H;
manifest.generator = 'oracle/refrun/golden_harness_modulate.js';

// [samplesPerBit, sampleRate, baudRate, mark, space]: tones below Nyquist; 4800 baud with the XModem exchange's pair
const RATES = [
  [5, 48000, 9600, 9600, 14400], [10, 48000, 4800, 9600, 14400], [20, 48000, 2400, 2400, 4800], [31, 48000, 1548, 1200, 2200],
  [32, 48000, 1500, 1200, 2200], [33, 48000, 1454, 1200, 2200], [40, 48000, 1200, 1200, 2200], [64, 48000, 750, 1200, 2200],
  [147, 44100, 300, 1070, 1270]];
const FRAMINGS = [
  ['8n1', {}],
  ['even_stop2', { parity: 'even', stopBits: 2 }],
  ['odd_start2', { parity: 'odd', startBits: 2 }],
  ['nopre', { preamblePattern: [], sfdPattern: [] }],       // (never with an empty payload: that is golden.npz's default_noframe_empty)
  ['pre4', { preamblePattern: [0xAA, 0x55, 0xAA, 0x55] }]];
const SEVEN = [0x00, 0xFF, 0x55, 0xA7, 0x01, 0x80, 0x3C];
const ONE = [0x00, 0xFF, 0x55];

function coreFor(cfg, spb) {
  const core = mkCore(cfg);
  const c = Object.assign({}, R.DEFAULT_FSK_CONFIG, cfg);
  if (core.params.samplesPerBit !== spb || Math.floor(c.sampleRate / c.baudRate) !== spb) throw new Error('samplesPerBit of ' + JSON.stringify(cfg) + ' is not ' + spb);
  if (!(Math.max(c.markFrequency, c.spaceFrequency) < c.sampleRate / 2)) throw new Error('tone at or above Nyquist');
  return core;
}

// the bits of a frame in the reference's order (fsk.ts:408-422), for the harness's own phase count
function frameBits(c, bytes) {
  const bits = [];
  for (const b of bytes) {
    for (let i = 0; i < c.startBits; i++) bits.push(0);
    for (let i = 7; i >= 0; i--) bits.push((b >> i) & 1);
    if (c.parity !== 'none') {
      let p = 0;
      for (let i = 0; i < 8; i++) p ^= (b >> i) & 1;
      bits.push(c.parity === 'even' ? p : 1 - p);
    }
    for (let i = 0; i < c.stopBits; i++) bits.push(1);
  }
  return bits;
}
const HI = new DataView(new ArrayBuffer(8));
function highWord(x) { HI.setFloat64(0, x); return HI.getUint32(0) & 0x7fffffff; }
// Where fdlibm's sine leaves its medium range.  __ieee754_rem_pio2 takes the Cody-Waite path while the argument's high word is
// <= 0x413921fb, and its comment calls that "|x| ~<= 2^19*(pi/2)"; the word is that of 2^20 * pi/2 = 1 647 099.3.  Both are recorded:
// 'stated' cases pass 2^19 * pi/2 = 823 549.7, where nothing changes, 'actual' cases pass the high-word test itself.
const LIMITS = {
  stated: { value: 524288 * Math.PI / 2, beyond: (x) => x > 524288 * Math.PI / 2, target: 1.035 },
  actual: { value: 1048576 * Math.PI / 2, beyond: (x) => highWord(x) > 0x413921fb, target: 1.025 }};

// { n, cross, last }: the signal's length, the first sample whose phase is beyond the medium range, and the phase of the last tone sample
function phaseWalk(c, spb, payloadLen, payload, beyond) {
  const bytes = [...c.preamblePattern, ...c.sfdPattern, ...payload.subarray(0, payloadLen)];
  const bitsPerByte = 8 + c.startBits + c.stopBits + (c.parity !== 'none' ? 1 : 0);
  let phase = 0, idx = bytes.length > 0 ? 2 * spb : 0, cross = -1, last = 0;
  for (const bit of frameBits(c, bytes)) {
    const f = bit === 1 ? c.markFrequency : c.spaceFrequency;
    for (let i = 0; i < spb; i++) {
      if (cross < 0 && beyond(phase)) cross = idx;
      last = phase;
      idx++;
      phase += 2 * Math.PI * f / c.sampleRate;
    }
  }
  return { n: idx + bitsPerByte * spb, cross, last };
}

async function main() {
  // ---------------- short cases: every samples-per-bit value meets every framing; every payload length on both sides of 32 ----------------
  const mods = [];
  for (let i = 0; i < RATES.length; i++) {
    const [spb, sampleRate, baudRate, markFrequency, spaceFrequency] = RATES[i];
    for (let j = 0; j < FRAMINGS.length; j++) {
      const [tag, framing] = FRAMINGS[j];
      const cfg = Object.assign({ sampleRate, baudRate, markFrequency, spaceFrequency }, framing);
      let len = [0, 1, 7][(i + j) % 3];
      if (tag === 'nopre' && len === 0) len = [1, 7][i % 2];
      const payload = len === 1 ? [ONE[(i + j) % 3]] : SEVEN.slice(0, len).map((_, k) => SEVEN[(k + i + j) % 7]);
      const name = 'spb' + spb + '_' + tag + '_' + len;
      const sig = await coreFor(cfg, spb).modulateData(new Uint8Array(payload));
      mods.push({ name, config: cfg, samplesPerBit: spb, framing: tag, payload, n: sig.length, signal: saveArray('mod.' + name, sig) });
    }
  }
  manifest.modulate = mods;

  // ---------------- long cases, one per kernel and limit: the phase passes the limit by 2 to 5 % ----------------
  const TAIL_CAP = 32768;
  const longs = [];
  for (const [spb, baudRate, which] of [[10, 4800, 'stated'], [32, 1500, 'stated'], [10, 4800, 'actual'], [32, 1500, 'actual']]) {
    const lim = LIMITS[which], LIMIT = lim.value;
    const cfg = { sampleRate: 48000, baudRate, markFrequency: 9600, spaceFrequency: 14400 };
    const c = Object.assign({}, R.DEFAULT_FSK_CONFIG, cfg);
    const core = coreFor(cfg, spb);
    const rand = rng32(0x10C0DE + spb + (which === 'actual' ? 1000 : 0));
    const pool = new Uint8Array(16384);
    for (let k = 0; k < pool.length; k++) pool[k] = Math.floor(rand() * 256);
    // the shortest payload whose last phase is lim.target times the limit (bisection: the phase grows with the length)
    let lo = 0, hi = pool.length;
    while (lo < hi) {
      const mid = (lo + hi) >> 1;
      if (phaseWalk(c, spb, mid, pool, lim.beyond).last >= lim.target * LIMIT) hi = mid; else lo = mid + 1;
    }
    const w = phaseWalk(c, spb, lo, pool, lim.beyond);
    const sig = await core.modulateData(pool.subarray(0, lo));
    const tones_end = sig.length - core.params.bitsPerByte * spb;
    if (sig.length !== w.n || w.cross < 0) throw new Error('phase walk disagrees with the reference: ' + sig.length + ' ' + JSON.stringify(w));
    if (!(w.last >= 1.02 * LIMIT && w.last <= 1.05 * LIMIT)) throw new Error('final phase ' + w.last / LIMIT + ' of the limit');
    if (sig.length - w.cross > TAIL_CAP) throw new Error('tail of ' + (sig.length - w.cross) + ' samples');
    const prefix = sig.subarray(0, w.cross);
    const name = 'long_' + which + '_spb' + spb;
    longs.push({
      name, config: cfg, samplesPerBit: spb, limit: which, limit_value: LIMIT, payload: saveArray('modlong.' + name + '.payload', pool.slice(0, lo)), n: sig.length,
      cross: w.cross, tones_end, final_phase: w.last, final_phase_over_limit: w.last / LIMIT,
      prefix_sha256: crypto.createHash('sha256').update(Buffer.from(prefix.buffer, prefix.byteOffset, prefix.byteLength)).digest('hex'),
      tail: saveArray('modlong.' + name + '.tail', sig.slice(w.cross))
    });
  }
  manifest.modulate_long = longs;
  manifest.arrays = arrays;
  fs.writeFileSync(path.join(H.OUT, 'manifest.json'), JSON.stringify(manifest));
  console.log('modulate cases', mods.length, '+', longs.length, 'long; arrays', Object.keys(arrays).length);
}
main().catch((e) => { console.error(e); process.exit(1); });
