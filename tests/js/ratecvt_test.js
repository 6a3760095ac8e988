'use strict';
// CaptureConverter / PlaybackConverter of napi/filters.js through the N-API addon (include/fskhip_next.h: fskhip_ratecvt_*).
//   cpu: the surface, the ratio and the default design, and the refusals that need no device.
//   gpu <capture digest> <playback digest>: one case per direction against the sha256 of what the Python binding returns for the
//        same inputs (formulas shared with tests/test_node_ratecvt.py, no random numbers) -- 66 streams, 44.1 kHz <-> 48 kHz, the
//        default 2 561 taps; capture: mu-law frames in two calls of 2 and 1 periods of 147; playback: 4 periods of 160 floats per
//        stream into s16 with ragged lengths; each digest covers the samples and the history rows behind them.  Then state /
//        setState, reset, the refusal of a bad nIn, and close.
// usage: node ratecvt_test.js cpu | gpu <capture> <playback>
const assert = require('assert');
const crypto = require('crypto');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

const S = 66;

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
  for (const C of [F.CaptureConverter, F.PlaybackConverter]) {
    assert.strictEqual(typeof C, 'function');
    for (const m of ['process', 'reset', 'state', 'setState', 'close', 'outCount']) assert.strictEqual(typeof C.prototype[m], 'function', m);
    assert.deepStrictEqual(C.ratio(44100, 48000), { up: 160, down: 147 });
    assert.deepStrictEqual(C.ratio(48000, 44100), { up: 147, down: 160 });
    assert.deepStrictEqual(C.ratio(8000, 48000), { up: 6, down: 1 });
    assert.strictEqual(C.defaultTaps(44100, 48000).length, 2561);
    assert.throws(() => C.ratio(44100.5, 48000), /rates must be positive whole numbers/);
    assert.throws(() => new C(8000, 44100, 4), /needs 7057 taps, the limit is 4096/);
    assert.throws(() => new C(1, 300, 4, { taps: [1] }), /ratio 300 \/ 1 outside 1\.\.256/);
    assert.throws(() => new C(3, 2, 0, { taps: [1] }), /zero n_streams or n_taps/);
    assert.throws(() => new C(3, 2, 4, { taps: [1], precision: 7 }), /unknown precision 7/);
    assert.throws(() => new C(3, 2, 4, { taps: new Array(4097).fill(0.1) }), /4097 taps do not fit/);
  }
  assert.strictEqual(typeof F.PlaybackConverter.prototype.outLength, 'function');
  console.log('js ratecvt cpu tests ok');
}

function gpuTests(wantCapture, wantPlayback) {
  const cap = new F.CaptureConverter(44100, 48000, S);
  assert.strictEqual(cap.taps.length, 2561);
  assert.deepStrictEqual([cap.up, cap.down, cap.history, cap.outCount(294)], [160, 147, 16, 320]);
  let h = crypto.createHash('sha256');
  const a = cap.process(mulawFrames(0, 294), 'mulaw', 'sample'), b = cap.process(mulawFrames(294, 147), 'mulaw', 'sample');
  assert.ok(a instanceof Float32Array && a.length === S * 320 && b.length === S * 160);
  h.update(bytesOf(a)); h.update(bytesOf(b)); h.update(bytesOf(cap.state()));
  assert.strictEqual(h.digest('hex'), wantCapture, 'capture: the Python binding computes something else');
  assert.throws(() => cap.process(new Int16Array(S * 147), 'mulaw'), /takes a Uint8Array/);
  assert.throws(() => cap.process(new Uint8Array(S * 147 + 1), 'mulaw'), /not a multiple of the stream count/);
  assert.throws(() => cap.process(new Uint8Array(S * 147), 'pcm24'), /unknown sample format/);
  // a bad nIn is the library's refusal and leaves the history as it was
  const before = cap.state();
  assert.throws(() => cap.process(new Uint8Array(S * 148), 'mulaw'), /n_in 148 is not a multiple of the down factor 147/);
  assert.deepStrictEqual(cap.state(), before);
  // setState(state()) on a twin continues as the original does; reset() zeroes
  const twin = new F.CaptureConverter(44100, 48000, S);
  twin.setState(cap.state());
  assert.deepStrictEqual(twin.process(mulawFrames(441, 147), 'mulaw', 'sample'), cap.process(mulawFrames(441, 147), 'mulaw', 'sample'));
  cap.reset();
  assert.ok(cap.state().every((v) => v === 0) && cap.state().length === S * 16);
  assert.throws(() => twin.setState(new Float32Array(3)), /state must be/);
  twin.close();
  cap.close();
  assert.throws(() => cap.state(), /destroyed/);

  const play = new F.PlaybackConverter(48000, 44100, S);
  assert.deepStrictEqual([play.up, play.down, play.history, play.outCount(640), play.outLength(1), play.outLength(0)], [147, 160, 18, 588, 17, 0]);
  const lens = Uint32Array.from({ length: S }, (_, s) => (s * 53) % 700);
  const y = play.process(floats(640), 's16', 'stream', lens);
  assert.ok(y instanceof Int16Array && y.length === S * 588);
  h = crypto.createHash('sha256');
  h.update(bytesOf(y)); h.update(bytesOf(play.state()));
  assert.strictEqual(h.digest('hex'), wantPlayback, 'playback: the Python binding computes something else');
  for (let s = 0; s < S; s++) for (let k = play.outLength(Math.min(lens[s], 640)); k < 588; k++) assert.strictEqual(y[s * 588 + k], 0, 'silence behind stream ' + s);
  const held = play.state();
  assert.throws(() => play.process(new Float32Array(S * 167), 's16'), /n_in 167 is not a multiple of the down factor 160/);
  assert.deepStrictEqual(play.state(), held);
  const frames = play.process(floats(160), 'mulaw', 'sample');
  assert.ok(frames instanceof Uint8Array && frames.length === 147 * S);
  const twinP = new F.PlaybackConverter(48000, 44100, S);
  twinP.setState(play.state());
  assert.deepStrictEqual(twinP.process(floats(320), 'alaw'), play.process(floats(320), 'alaw'));
  play.reset(3);
  const st = play.state();
  assert.ok(st.subarray(3 * 18, 4 * 18).every((v) => v === 0) && st.subarray(4 * 18, 5 * 18).some((v) => v !== 0));
  twinP.close();
  play.close();
  console.log('js ratecvt gpu tests ok');
}

const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') gpuTests(process.argv[3], process.argv[4]); else cpuTests();
