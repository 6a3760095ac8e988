'use strict';
// Upsampler / Downsampler of napi/filters.js through the N-API addon (include/fskhip_next.h: fskhip_resampler_*).
//   cpu: the surface, and the refusals that need no device.
//   gpu <up digest> <down digest>: one case per direction against the sha256 of what the Python binding returns for the same
//        inputs (formulas shared with tests/test_node_resample.py, no random numbers) -- 66 streams, factor 6, the default 97
//        taps; up: mu-law frames in two calls of 60 and 40 samples; down: 600 floats per stream into s16 with ragged lengths;
//        each digest covers the samples and the history rows behind them.  Then reset, setState and close.
// usage: node resample_test.js cpu | gpu <up> <down>
const assert = require('assert');
const crypto = require('crypto');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

const S = 66, L = 6;

function bytesOf(a) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength); }
function mulawFrames(m0, n) {                 // frames [n][S]
  const a = new Uint8Array(n * S);
  for (let m = 0; m < n; m++) for (let s = 0; s < S; s++) a[m * S + s] = (s * 37 + (m0 + m) * 11 + ((m0 + m) * (m0 + m)) % 7) & 0xff;
  return a;
}
function floats(n) {                          // [S][n]
  const a = new Float32Array(S * n);
  for (let s = 0; s < S; s++) for (let t = 0; t < n; t++) a[s * n + t] = ((s * 131 + t * 29) % 2001 - 1000) / 1000;
  return a;
}

function cpuTests() {
  for (const C of [F.Upsampler, F.Downsampler]) {
    assert.strictEqual(typeof C, 'function');
    for (const m of ['process', 'reset', 'state', 'setState', 'close']) assert.strictEqual(typeof C.prototype[m], 'function', m);
    assert.throws(() => new C(33, 4), /factor 33 outside 1\.\.32/);
    assert.throws(() => new C(0, 4), /factor 0 outside 1\.\.32/);
    assert.throws(() => new C(6, 0), /zero n_streams or n_taps/);
    assert.throws(() => new C(6, 4, { precision: 7 }), /unknown precision 7/);
    assert.throws(() => new C(6, 4, { taps: new Array(4097).fill(0.1) }), /4097 taps do not fit/);
  }
  console.log('js resample cpu tests ok');
}

function gpuTests(wantUp, wantDown) {
  const up = new F.Upsampler(L, S);
  assert.strictEqual(up.taps.length, 97);
  assert.strictEqual(up.history, 16);
  let h = crypto.createHash('sha256');
  const a = up.process(mulawFrames(0, 60), 'mulaw', 'sample'), b = up.process(mulawFrames(60, 40), 'mulaw', 'sample');
  assert.ok(a instanceof Float32Array && a.length === S * 360 && b.length === S * 240);
  h.update(bytesOf(a)); h.update(bytesOf(b)); h.update(bytesOf(up.state()));
  assert.strictEqual(h.digest('hex'), wantUp, 'up: the Python binding computes something else');
  assert.throws(() => up.process(new Int16Array(S), 'mulaw'), /takes a Uint8Array/);
  assert.throws(() => up.process(new Uint8Array(S + 1), 'mulaw'), /not a multiple of the stream count/);
  assert.throws(() => up.process(new Uint8Array(S), 'pcm24'), /unknown sample format/);
  // setState(state()) on a twin continues as the original does; reset() zeroes
  const twin = new F.Upsampler(L, S);
  twin.setState(up.state());
  assert.deepStrictEqual(twin.process(mulawFrames(100, 7), 'mulaw', 'sample'), up.process(mulawFrames(100, 7), 'mulaw', 'sample'));
  up.reset();
  assert.ok(up.state().every((v) => v === 0) && up.state().length === S * 16);
  assert.throws(() => twin.setState(new Float32Array(3)), /state must be/);
  twin.close();
  up.close();
  assert.throws(() => up.state(), /destroyed/);

  const down = new F.Downsampler(L, S);
  assert.strictEqual(down.history, 96);
  const lens = Uint32Array.from({ length: S }, (_, s) => (s * 53) % 700);
  const y = down.process(floats(600), 's16', 'stream', lens);
  assert.ok(y instanceof Int16Array && y.length === S * 100);
  h = crypto.createHash('sha256');
  h.update(bytesOf(y)); h.update(bytesOf(down.state()));
  assert.strictEqual(h.digest('hex'), wantDown, 'down: the Python binding computes something else');
  for (let s = 0; s < S; s++) for (let k = Math.ceil((lens[s] + 96) / L); k < 100; k++) assert.strictEqual(y[s * 100 + k], 0, 'silence behind stream ' + s);
  const before = down.state();
  assert.throws(() => down.process(new Float32Array(S * 7), 's16'), /n_in 7 is not a multiple of the factor 6/);
  assert.deepStrictEqual(down.state(), before);
  down.close();
  console.log('js resample gpu tests ok');
}

const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') gpuTests(process.argv[3], process.argv[4]); else cpuTests();
