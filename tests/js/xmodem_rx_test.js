'use strict';
// XModemReceiverBatch through the N-API addon (include/fskhip_next.h: fskhip_xmodem_rx_*).
// cpu: the argument checks, which are made before the library is called, and the addon's own refusal of a handle that is none.
// gpu: a batch whose rings hold complete packets (two serialised packets per stream, some streams silent, demodulated from samples)
// is cloned (remap with the identity); poll() on one clone lists exactly the streams for which scanBursts over demodulate() of the
// other finds packets, with the same ten result words and the same payloads; the state follows, the rings are empty afterwards.
// usage: node xmodem_rx_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

function cpuTests() {
  for (const m of ['poll', 'reset', 'state', 'setState', 'close']) assert.strictEqual(typeof X.XModemReceiverBatch.prototype[m], 'function');
  for (const f of ['xmodemRxCreate', 'xmodemRxDestroy', 'xmodemRxPoll', 'xmodemRxReset', 'xmodemRxState', 'xmodemRxSetState']) assert.strictEqual(typeof addon[f], 'function');
  assert.throws(() => new X.XModemReceiverBatch(null), /processor must be an FSKProcessorBatch/);
  assert.throws(() => new X.XModemReceiverBatch({ nStreams: 4, handle: null }), /processor destroyed/);
  const b = Object.create(X.XModemReceiverBatch.prototype);   // no device here: the checks come before the handle is used
  b.nStreams = 4; b.handle = null;
  assert.throws(() => b.poll(null), /options must be an object/);
  assert.throws(() => b.poll(7), /options must be an object/);
  assert.throws(() => b.poll({ mask: 5 }), /mask must be an array/);
  assert.throws(() => b.poll({ mask: [true, false] }), /one entry per stream \(4\)/);
  assert.throws(() => b.poll({ mask: new Uint8Array(5) }), /one entry per stream \(4\)/);
  assert.throws(() => b.reset(1.5), /stream must be an integer/);
  assert.throws(() => b.setState(null), /state must be an object/);
  assert.throws(() => b.setState({ expected: 3 }), /expected must be an array/);
  assert.throws(() => b.setState({ packets: [1, 2] }), /packets must have one entry per stream \(4\)/);
  assert.throws(() => b.setState({ dropped: [1, 2, -1, 0] }), /dropped must hold integers/);
  // past the checks the calls reach the addon, which refuses what is no receiver handle
  assert.throws(() => b.poll(), /receiver destroyed/);
  assert.throws(() => b.poll({ mask: [1, 0, 0, 1] }), /receiver destroyed/);
  assert.throws(() => b.reset(), /receiver destroyed/);
  assert.throws(() => b.state(), /receiver destroyed/);
  assert.throws(() => b.setState({ expected: [1, 2, 3, 4] }), /receiver destroyed/);
  assert.throws(() => addon.xmodemRxPoll(), /too few arguments/);
  b.close();   // nothing to close
  console.log('js xmodem rx cpu tests ok');
}

function gpuTests() {
  const S = 70, Q = 4096;
  const sent = Array.from({ length: S }, (_, s) => [0, 1].map((k) => Uint8Array.from({ length: (s + 3 * k) % 8 }, (_v, j) => (s * 29 + j * 7 + k) & 0xff)));
  const wires = sent.map((two) => { const w = X.serializeBatch([1, 2], two); const o = new Uint8Array(w[0].length + w[1].length); o.set(w[0]); o.set(w[1], w[0].length); return o; });
  const mod = new M.FSKBatch(S, {});
  const frames = mod.modulateData(wires);
  mod.close();
  let longest = 0;
  for (const f of frames) longest = Math.max(longest, f.length);
  const quanta = Math.ceil(longest / Q) + 4;   // (silence behind the signal flushes the last byte)
  const silent = (s) => s % 5 === 0;           // these rings stay empty
  const src = new P.FSKProcessorBatch(new M.FSKBatch(S, {}), {});
  for (let q = 0; q < quanta; q++) {
    const inp = new Float32Array(S * Q);
    for (let s = 0; s < S; s++) if (!silent(s) && q * Q < frames[s].length) inp.set(frames[s].subarray(q * Q, Math.min(frames[s].length, (q + 1) * Q)), s * Q);
    src.process(inp, Q, 0);
  }
  const all = Array.from({ length: S }, (_, s) => s);
  const polled = src.remap(all), dense = src.remap(all);
  const want = X.scanBursts(dense.demodulate(), 1);
  const listed = all.filter((s) => want[s].status !== 0 || want[s].packets + want[s].dropped > 0);
  assert.deepStrictEqual(listed, all.filter((s) => !silent(s)));
  const rx = new X.XModemReceiverBatch(polled);
  assert.deepStrictEqual(Array.from(rx.state().expected), all.map(() => 1));
  const r = rx.poll();
  assert.ok(r.streams instanceof Uint32Array && r.offsets instanceof Uint32Array && r.data instanceof Uint8Array);
  assert.deepStrictEqual(Array.from(r.streams), listed);
  assert.strictEqual(r.offsets[0], 0);
  assert.strictEqual(r.offsets[listed.length], r.data.length);
  listed.forEach((s, i) => {
    assert.deepStrictEqual(r.results[i], want[s], 'stream ' + s);   // the ten words and the payload
    assert.strictEqual(want[s].statusName, 'need_more');
    assert.deepStrictEqual(Array.from(r.data.subarray(r.offsets[i], r.offsets[i + 1])), Array.from(sent[s][0]).concat(Array.from(sent[s][1])), 'stream ' + s);
  });
  const st = rx.state();
  assert.deepStrictEqual(Array.from(st.expected), all.map((s) => want[s].expectedAfter));
  assert.deepStrictEqual(Array.from(st.packets), all.map((s) => (silent(s) ? 0 : 2)));
  assert.deepStrictEqual(Array.from(st.dropped), all.map(() => 0));
  assert.deepStrictEqual(Array.from(polled.rxLengths()), all.map(() => 0));   // whole packets only: nothing waits
  const none = rx.poll({ mask: all.map(() => true) });
  assert.deepStrictEqual([none.streams.length, none.results.length, Array.from(none.offsets), none.data.length], [0, 0, [0], 0]);
  // state: set, reset one, reset all; a sequence number out of range is refused by name
  rx.setState({ expected: all.map((s) => 1 + (s % 255)), packets: all.map((s) => s) });
  assert.deepStrictEqual(Array.from(rx.state().expected), all.map((s) => 1 + (s % 255)));
  assert.throws(() => rx.setState({ expected: all.map((s) => (s === 9 ? 256 : 1)) }), /expected\[9\] = 256 is not a sequence number/);
  rx.reset(3);
  assert.deepStrictEqual(Array.from(rx.state().expected), all.map((s) => (s === 3 ? 1 : 1 + (s % 255))));
  rx.reset();
  assert.deepStrictEqual(Array.from(rx.state().expected), all.map(() => 1));
  assert.deepStrictEqual(Array.from(rx.state().packets), all);   // the counters stay
  assert.throws(() => addon.processorRemap(polled.handle, src.handle, all), /used already/);   // a polled processor is a used one
  rx.close();
  assert.throws(() => rx.poll(), /receiver destroyed/);
  for (const b of [polled, dense, src]) { b.close(); b.batch.close(); }
  console.log('js xmodem rx gpu tests ok');
}

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
