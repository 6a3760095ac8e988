'use strict';
// The rate converters' calls of any length through the N-API addon (include/fskhip_next.h: "Rate conversion in calls of any length";
// napi/filters.js: processAny, position, setPosition, outCountAny, inCountAny; napi/fsk-processor.js: processSamplesAtAny).
//   cpu: the surface, without a device.
//   gpu <capture digest> <playback digest>: 66 streams, 44.1 kHz <-> 48 kHz, the default 2 561 taps, inputs by formulas shared with
//        tests/test_node_ratecvt_any.py (no random numbers).  processAny over cuts of 128, 1, 129 ... equals one call, sample for
//        sample, with the same state and position, and that one call's sha256 (samples, history rows, position) is the Python
//        binding's; position / setPosition carry a handle by hand; a call that writes nothing moves the position; then
//        processSamplesAtAny in 128-frame quanta against the chain processAny -> process() -> processAny on twins.
// usage: node ratecvt_any_test.js cpu | gpu <capture> <playback>
const assert = require('assert');
const crypto = require('crypto');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

const S = 66;
const CUTS = [128, 1, 129, 128, 146, 1, 148, 128];        // 809 inputs: no whole number of periods of 147 or 160

function bytesOf(a) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength); }
function mulawFrames(m0, n) {                 // frames [n][S]
  const a = new Uint8Array(n * S);
  for (let m = 0; m < n; m++) for (let s = 0; s < S; s++) a[m * S + s] = (s * 37 + (m0 + m) * 11 + ((m0 + m) * (m0 + m)) % 7) & 0xff;
  return a;
}
function floats(t0, n) {                      // [S][n], columns t0 .. t0 + n - 1 of the signal
  const a = new Float32Array(S * n);
  for (let s = 0; s < S; s++) for (let t = 0; t < n; t++) a[s * n + t] = ((s * 131 + (t0 + t) * 29) % 2001 - 1000) / 1000;
  return a;
}
// [S][n] pieces side by side -> [S][sum n]
function joinRows(parts) {
  const total = parts.reduce((a, p) => a + p.length / S, 0), out = new parts[0].constructor(S * total);
  let at = 0;
  for (const p of parts) {
    const n = p.length / S;
    for (let s = 0; s < S; s++) out.set(p.subarray(s * n, (s + 1) * n), s * total + at);
    at += n;
  }
  return out;
}
function u32(n) { const b = Buffer.alloc(4); b.writeUInt32LE(n); return b; }

function cpuTests() {
  for (const C of [F.CaptureConverter, F.PlaybackConverter]) {
    for (const m of ['processAny', 'setPosition', 'outCountAny', 'inCountAny']) assert.strictEqual(typeof C.prototype[m], 'function', m);
    assert.strictEqual(typeof Object.getOwnPropertyDescriptor(Object.getPrototypeOf(C.prototype), 'position').get, 'function');
  }
  const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
  assert.strictEqual(typeof P.FSKProcessorBatch.prototype.processSamplesAtAny, 'function');
  console.log('js ratecvt any cpu tests ok');
}

function gpuTests(wantCapture, wantPlayback) {
  const N = CUTS.reduce((a, b) => a + b, 0);
  // capture: mu-law frames
  const one = new F.CaptureConverter(44100, 48000, S), cut = new F.CaptureConverter(44100, 48000, S);
  assert.deepStrictEqual([one.position, one.outCountAny(128), one.inCountAny(140), one.outCountAny(0)], [0, 140, 128, 0]);
  const whole = one.processAny(mulawFrames(0, N), 'mulaw', 'sample');
  assert.ok(whole instanceof Float32Array && whole.length === S * Math.ceil(N * 160 / 147) && one.position === N % 147);
  let h = crypto.createHash('sha256');
  h.update(bytesOf(whole)); h.update(bytesOf(one.state())); h.update(u32(one.position));
  assert.strictEqual(h.digest('hex'), wantCapture, 'capture: the Python binding computes something else');
  let parts = [], at = 0;
  for (const n of CUTS) {
    const want = cut.outCountAny(n), y = cut.processAny(mulawFrames(at, n), 'mulaw', 'sample');
    assert.strictEqual(y.length, S * want);
    parts.push(y);
    at += n;
    assert.strictEqual(cut.position, at % 147);
  }
  assert.deepStrictEqual(joinRows(parts), whole);
  assert.deepStrictEqual(cut.state(), one.state());
  // carried by hand: state and position
  const twin = new F.CaptureConverter(44100, 48000, S);
  twin.setState(one.state());
  twin.setPosition(one.position);
  assert.strictEqual(twin.position, one.position);
  assert.deepStrictEqual(twin.processAny(mulawFrames(N, 200), 'mulaw', 'sample'), one.processAny(mulawFrames(N, 200), 'mulaw', 'sample'));
  assert.throws(() => twin.setPosition(147), /position 147 outside 0\.\.146/);
  assert.throws(() => twin.setPosition(-1), /outside/);
  // the whole-period call still wants its multiple, works from any position and leaves it
  const pos = one.position;
  assert.ok(pos !== 0);
  assert.throws(() => one.process(mulawFrames(0, 148), 'mulaw', 'sample'), /n_in 148 is not a multiple of the down factor 147/);
  assert.deepStrictEqual(one.process(mulawFrames(7, 147), 'mulaw', 'sample'), twin.processAny(mulawFrames(7, 147), 'mulaw', 'sample'));
  assert.strictEqual(one.position, pos);
  one.reset(2);
  assert.strictEqual(one.position, pos);
  one.reset();
  assert.strictEqual(one.position, 0);
  for (const c of [one, cut, twin]) c.close();

  // playback: floats into s16 rows; 147 / 160 has calls that write nothing
  const pone = new F.PlaybackConverter(48000, 44100, S), pcut = new F.PlaybackConverter(48000, 44100, S);
  assert.deepStrictEqual([pone.outCountAny(128), pone.inCountAny(128), pone.outCountAny(1)], [118, 139, 1]);
  const pwhole = pone.processAny(floats(0, N), 's16', 'stream');
  assert.ok(pwhole instanceof Int16Array && pwhole.length === S * Math.ceil(N * 147 / 160) && pone.position === N % 160);
  h = crypto.createHash('sha256');
  h.update(bytesOf(pwhole)); h.update(bytesOf(pone.state())); h.update(u32(pone.position));
  assert.strictEqual(h.digest('hex'), wantPlayback, 'playback: the Python binding computes something else');
  parts = []; at = 0;
  let empty = 0;
  for (const n of [12, 1, ...CUTS.slice(0, -1), CUTS[CUTS.length - 1] - 13]) {   // (12 * 147 / 160 = 11.025: one input at position 12 writes nothing)
    const want = pcut.outCountAny(n), before = pcut.position, y = pcut.processAny(floats(at, n), 's16', 'stream');
    assert.strictEqual(y.length, S * want);
    if (want === 0) { empty++; assert.strictEqual(pcut.position, before + 1); } else parts.push(y);
    at += n;
  }
  assert.ok(empty >= 1 && at === N);
  assert.deepStrictEqual(joinRows(parts), pwhole);
  assert.deepStrictEqual(pcut.state(), pone.state());
  assert.strictEqual(pcut.position, pone.position);
  pone.close(); pcut.close();

  // the streaming quantum: 128 frames in and out at 44.1 kHz, 1 and 129 mixed in, against the chain on twins
  const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
  const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
  const batches = [0, 1].map(() => new M.FSKBatch(S, {}));
  const procs = batches.map((b) => new P.FSKProcessorBatch(b));
  const caps = [0, 1].map(() => new F.CaptureConverter(44100, 48000, S)), plays = [0, 1].map(() => new F.PlaybackConverter(48000, 44100, S));
  const payloads = Array.from({ length: S }, (_, s) => Uint8Array.from([0x41 + s % 26, s]));
  for (const p of procs) p.modulate(payloads);
  let wire = null;
  [128, 128, 1, 129, 128, 129, 1, 128].forEach((nOut, k) => {
    const nIn = wire ? wire.length / S : 0;
    // the chain: processAny -> process() with the engine counts the handles give (a side with none left out) -> processAny
    let x = wire ? caps[0].processAny(wire, 's16', 'sample') : null;
    if (x && x.length === 0) x = null;
    const nEng = plays[0].inCountAny(nOut);
    const y = procs[0].process(x, x ? x.length / S : 0, nEng);
    const want = plays[0].processAny(y, 's16', 'sample');
    const got = procs[1].processSamplesAtAny(wire, { format: 's16', layout: 'sample', nIn, upsampler: caps[1] },
      { format: 's16', layout: 'sample', nOut, downsampler: plays[1] });
    assert.ok(got instanceof Int16Array && got.length === S * nOut, 'quantum ' + k);
    assert.deepStrictEqual(got, want, 'quantum ' + k);
    assert.deepStrictEqual(caps[1].state(), caps[0].state());
    assert.deepStrictEqual(plays[1].state(), plays[0].state());
    assert.deepStrictEqual([caps[1].position, plays[1].position], [caps[0].position, plays[0].position]);
    assert.deepStrictEqual(procs[1].txState(), procs[0].txState());
    wire = want;
  });
  assert.ok(wire.some((v) => v !== 0));
  const up = new F.Upsampler(6, S);
  assert.throws(() => procs[1].processSamplesAtAny(new Uint8Array(S * 8), { nIn: 8, upsampler: up }), /processSamplesAtAny: upsampler is a Upsampler/);
  up.close();
  for (const o of [...caps, ...plays, ...procs, ...batches]) o.close();
  console.log('js ratecvt any gpu tests ok');
}

const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') gpuTests(process.argv[3], process.argv[4]); else cpuTests();
