'use strict';
// FSKProcessorBatch.processSamplesAt with a CaptureConverter / PlaybackConverter through the N-API addon (include/fskhip_next.h,
// fskhip_processor_process_ratecvt_host).
//   cpu  converters pass the checks of napi/fsk-processor.js up to the addon's call; the three new throws -- one of each kind, the
//        two counts that are no whole periods -- and the existing ones in their words
//   gpu  one quantum at 44.1 kHz, mu-law frames of 441: what processSamplesAt sends, the playback converter's history behind it, and
//        the capture converter's history after a second processor took those frames equal what the Python host got for the same
//        calls (the file named on the command line, written by tests/test_node_processor_ratecvt.py); and both equal the chain
//        PlaybackConverter.process over process() on a twin
// usage: node processor_ratecvt_test.js cpu | gpu <expected.json>
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

function cpuTests() {
  const b = Object.create(P.FSKProcessorBatch.prototype);      // the checks need the stream count only
  Object.assign(b, { nStreams: 3, flags: 0, handle: null, processDemodulationCallCount: 0 });
  const fake = (kind, nStreams, up, down) => Object.assign(Object.create(kind.prototype), { nStreams, handle: null, up, down });
  const cap = fake(F.CaptureConverter, 3, 160, 147), play = fake(F.PlaybackConverter, 3, 147, 160);
  const up = fake(F.Upsampler, 3), down = fake(F.Downsampler, 3);
  const frames = new Uint8Array(3 * 294);
  // accepted: the next refusal is the addon's own, of the processor that is not there
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294, upsampler: cap }, { nOut: 441, downsampler: play }), /processor destroyed/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 147, upsampler: cap }), /processor destroyed/);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 147, downsampler: play }), /processor destroyed/);
  assert.strictEqual(b.processDemodulationCallCount, 2);
  b.processDemodulationCallCount = 0;
  // one call, one kind
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294, upsampler: cap }, { nOut: 8, downsampler: down }),
    (e) => e instanceof TypeError && /CaptureConverter.*Downsampler.*not one of each/.test(e.message));
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8, upsampler: up }, { nOut: 147, downsampler: play }),
    (e) => e instanceof TypeError && /Upsampler.*PlaybackConverter.*not one of each/.test(e.message));
  // whole periods
  assert.throws(() => b.processSamplesAt(frames, { nIn: 293, upsampler: cap }),
    (e) => e instanceof RangeError && /293 samples per stream are not a multiple of the converter's down factor 147/.test(e.message));
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294, upsampler: cap }, { nOut: 440, downsampler: play }),
    (e) => e instanceof RangeError && /nOut 440 is not a multiple of the converter's up factor 147/.test(e.message));
  // the existing throws, in their words: a converter of the other direction is no more welcome than a resampler of it
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294, upsampler: play }), /upsampler must be an Upsampler/);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 147, downsampler: cap }), /downsampler must be an Downsampler/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294 }, { nOut: 147, downsampler: play }), /upsampler must be an Upsampler/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 294, upsampler: fake(F.CaptureConverter, 4, 160, 147) }), /upsampler has 4 streams, the batch 3/);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 147, downsampler: fake(F.PlaybackConverter, 2, 147, 160) }), /downsampler has 2 streams, the batch 3/);
  assert.strictEqual(b.processDemodulationCallCount, 0);
  console.log('js processor ratecvt cpu tests ok');
}

function gpuTests(expectedPath) {
  const want = JSON.parse(fs.readFileSync(expectedPath, 'utf8'));
  const S = want.streams, Q = want.quantum;
  const hex = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex');
  const mk = () => { const batch = new M.FSKBatch(S, {}); return { batch, proc: new P.FSKProcessorBatch(batch) }; };
  const tx = mk(), rx = mk(), twin = mk();
  const play = new F.PlaybackConverter(48000, 44100, S), cap = new F.CaptureConverter(44100, 48000, S), playTwin = new F.PlaybackConverter(48000, 44100, S);
  assert.deepStrictEqual([play.up, play.down, cap.up, cap.down, play.history], [147, 160, 160, 147, 18]);
  const payloads = Array.from({ length: S }, (_, s) => Uint8Array.from(want.payloads[s]));
  tx.proc.modulate(payloads);
  twin.proc.modulate(payloads);
  let frames = null;
  for (let q = 0; q < want.quanta; q++) {
    frames = tx.proc.processSamplesAt(null, {}, { nOut: Q, downsampler: play });
    assert.ok(frames instanceof Uint8Array && frames.length === Q * S);
    const chain = playTwin.process(twin.proc.process(null, 0, Q / 147 * 160), 'mulaw', 'sample');
    assert.strictEqual(hex(frames), hex(chain), 'quantum ' + q + ' against the chain');
    assert.strictEqual(hex(play.state()), hex(playTwin.state()), 'quantum ' + q + ' history against the chain');
    assert.strictEqual(rx.proc.processSamplesAt(frames, { nIn: Q, upsampler: cap }), null);
  }
  assert.strictEqual(hex(frames), want.frames, 'the last quantum against the Python host');
  assert.strictEqual(hex(play.state()), want.play_state, 'the playback history against the Python host');
  assert.strictEqual(hex(cap.state()), want.cap_state, 'the capture history against the Python host');
  assert.strictEqual(rx.proc.snapshot().processor.toString('hex'), want.rx_processor, 'the receiving processor against the Python host');
  // the library's own refusals come through with their message
  assert.throws(() => M.addon.processorProcessSamplesAt(rx.proc.handle, play.handle, null, new Uint8Array(S * 147), 2, 1, 147, S, 2, 1, 0, S, 0),
    /the capture handle converts for playback/);
  assert.throws(() => M.addon.processorProcessSamplesAt(rx.proc.handle, cap.handle, null, new Uint8Array(S * 147), 2, 1, 146, S, 2, 1, 0, S, 0),
    /n_in 146 is not a multiple of the capture handle's down factor 147/);
  for (const x of [play, cap, playTwin]) x.close();
  for (const x of [tx, rx, twin]) { x.proc.close(); x.batch.close(); }
  console.log('js processor ratecvt gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'cpu') cpuTests(); else gpuTests(process.argv[3]);
