'use strict';
// Which TX path a quantum ran, through the N-API addon (include/fskhip_next.h: fskhip_processor_last_tx_kernel;
// napi/fsk-processor.js: lastTxKernel, PROC_RATECVT_PAIR).
//   cpu: the surface, without a device.
//   gpu: 66 streams, 48 kHz engine, 44.1 kHz playback (147 / 160, the default 2 561 taps), the host forms.  processSamplesAtAny
//        stream-major names the fused any-length kernel and as frames the two launches; a twin under PROC_RATECVT_PAIR names the
//        two launches for both and writes the same samples, history and position; the other process forms name their kernels.
// usage: node processor_ratecvt_any_fused_test.js cpu | gpu
const assert = require('assert');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));

const S = 66;
const FUSED_ANY = 'processor_io_ratecvt_kernel<any>', FUSED = 'processor_io_ratecvt_kernel';
const PAIR_ANY = 'processor_io_kernel+ratecvt_playback_any_kernel';

function cpuTests() {
  assert.strictEqual(typeof Object.getOwnPropertyDescriptor(P.FSKProcessorBatch.prototype, 'lastTxKernel').get, 'function');
  assert.strictEqual(P.PROC_RATECVT_PAIR, 4);
  console.log('js processor ratecvt any fused cpu tests ok');
}

function gpuTests() {
  const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
  const batches = [0, 1].map(() => new M.FSKBatch(S, {}));
  const procs = batches.map((b) => new P.FSKProcessorBatch(b));
  procs[1].flags |= P.PROC_RATECVT_PAIR;
  const plays = [0, 1].map(() => new F.PlaybackConverter(48000, 44100, S));
  const payloads = Array.from({ length: S }, (_, s) => Uint8Array.from([0x41 + s % 26, s]));
  assert.strictEqual(procs[0].lastTxKernel, '');
  for (const p of procs) p.modulate(payloads);
  [[128, 'stream', 's16'], [1, 'stream', 'mulaw'], [129, 'sample', 's16'], [147, 'stream', 'alaw'], [128, 'sample', 'mulaw'], [2, 'stream', 'f32']].forEach(([nOut, layout, format], k) => {
    const got = procs[0].processSamplesAtAny(null, {}, { format, layout, nOut, downsampler: plays[0] });
    const want = procs[1].processSamplesAtAny(null, {}, { format, layout, nOut, downsampler: plays[1] });
    assert.strictEqual(procs[0].lastTxKernel, layout === 'stream' ? FUSED_ANY : PAIR_ANY, 'quantum ' + k);
    assert.strictEqual(procs[1].lastTxKernel, PAIR_ANY, 'quantum ' + k);
    assert.ok(got.length === S * nOut);
    assert.deepStrictEqual(got, want, 'quantum ' + k);
    assert.deepStrictEqual(plays[0].state(), plays[1].state());
    assert.strictEqual(plays[0].position, plays[1].position);
    assert.deepStrictEqual(procs[0].txState(), procs[1].txState());
  });
  // no TX side; then the other forms
  assert.strictEqual(procs[0].processSamplesAtAny(null, {}, { nOut: 0 }), null);
  assert.strictEqual(procs[0].lastTxKernel, '');
  const fresh = new F.PlaybackConverter(48000, 44100, S);
  procs[0].processSamplesAt(null, {}, { format: 's16', layout: 'stream', nOut: 147, downsampler: fresh });
  assert.strictEqual(procs[0].lastTxKernel, FUSED);
  procs[0].process(null, 0, 64);
  assert.strictEqual(procs[0].lastTxKernel, 'processor_io_kernel');
  procs[0].processSamples(null, {}, { format: 'mulaw', layout: 'sample', nOut: 64 });
  assert.strictEqual(procs[0].lastTxKernel, 'processor_io_fmt_kernel');
  fresh.close();
  for (const x of [...plays, ...procs, ...batches]) x.close();
  console.log('js processor ratecvt any fused gpu tests ok');
}

if (process.argv[2] === 'cpu') cpuTests();
else if (process.argv[2] === 'gpu') gpuTests();
else { console.error('usage: node processor_ratecvt_any_fused_test.js cpu | gpu'); process.exit(2); }
