'use strict';
// XModemSenderBatch through the N-API addon (include/fskhip_next.h: fskhip_xmodem_tx_*).
// cpu: the argument checks, which are made before the library is called, and the addon's own refusal of a handle that is none.
// gpu: the closed loop for three streams -- the sender on processor A, XModemReceiverBatch on processor B, A's output samples into B and
// B's into A quantum by quantum, the host sending the control byte each receiver record asks for: every file arrives byte-identical,
// every sender ends 'done', and the counters are those of a transfer without errors.
// usage: node xmodem_tx_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

function cpuTests() {
  for (const m of ['send', 'poll', 'reset', 'state', 'setState', 'close']) assert.strictEqual(typeof X.XModemSenderBatch.prototype[m], 'function');
  for (const f of ['xmodemTxCreate', 'xmodemTxDestroy', 'xmodemTxSend', 'xmodemTxPoll', 'xmodemTxReset', 'xmodemTxState', 'xmodemTxSetState']) assert.strictEqual(typeof addon[f], 'function');
  assert.throws(() => new X.XModemSenderBatch(null), /processor must be an FSKProcessorBatch/);
  assert.throws(() => new X.XModemSenderBatch({ nStreams: 4, handle: null }, null), /options must be an object/);
  for (const bad of [0, 256, 1.5, '16']) assert.throws(() => new X.XModemSenderBatch({ nStreams: 4, handle: null }, { maxPayloadSize: bad }), /maxPayloadSize must be an integer in 1\.\.255/);
  for (const bad of [-1, 0.5, 2 ** 32]) assert.throws(() => new X.XModemSenderBatch({ nStreams: 4, handle: null }, { maxRetries: bad }), /maxRetries must be an integer/);
  assert.throws(() => new X.XModemSenderBatch({ nStreams: 4, handle: null }), /processor destroyed/);
  const b = Object.create(X.XModemSenderBatch.prototype);   // no device here: the checks come before the handle is used
  b.nStreams = 4; b.handle = null;
  const files = [[1], [2], [], [3, 4]];
  assert.throws(() => b.send(7), /files must be an array/);
  assert.throws(() => b.send([[1], [2]]), /files must have one entry per stream \(4\)/);
  assert.throws(() => b.send(files, null), /options must be an object/);
  assert.throws(() => b.send(files, { mask: 5 }), /mask must be an array/);
  assert.throws(() => b.send(files, { mask: [1, 0] }), /mask must have one entry per stream \(4\)/);
  assert.throws(() => b.send([[1], 'x', [], []]), /files\[1\] must be a byte array/);
  assert.throws(() => b.poll(null), /options must be an object/);
  assert.throws(() => b.poll({ mask: 5 }), /mask must be an array/);
  assert.throws(() => b.poll({ abort: 'yes' }), /abort must be an array/);
  assert.throws(() => b.poll({ abort: [true] }), /abort must have one entry per stream \(4\)/);
  assert.throws(() => b.reset(1.5), /stream must be an integer/);
  assert.throws(() => b.setState(null), /state must be an object/);
  assert.throws(() => b.setState({ sequence: 3 }), /sequence must be an array/);
  assert.throws(() => b.setState({ fragmentIndex: [1, 2] }), /fragmentIndex must have one entry per stream \(4\)/);
  assert.throws(() => b.setState({ retransmitted: [1, 2, -1, 0] }), /retransmitted must hold integers/);
  // past the checks the calls reach the addon, which refuses what is no sender handle
  assert.throws(() => b.send(files), /sender destroyed/);
  assert.throws(() => b.send([null, [2], null, null], { mask: [0, 1, 0, 0] }), /sender destroyed/);   // entries of unselected streams are not looked at
  assert.throws(() => b.poll(), /sender destroyed/);
  assert.throws(() => b.poll({ mask: [1, 0, 0, 1], abort: [0, 0, 1, 0] }), /sender destroyed/);
  assert.throws(() => b.reset(), /sender destroyed/);
  assert.throws(() => b.state(), /sender destroyed/);
  assert.throws(() => b.setState({ state: [0, 0, 0, 0] }), /sender destroyed/);
  assert.throws(() => addon.xmodemTxPoll(), /too few arguments/);
  b.close();   // nothing to close
  console.log('js xmodem tx cpu tests ok');
}

function gpuTests() {
  const S = 3, Q = 512, ACK = 0x06, NAK = 0x15, maxPayloadSize = 16;
  const cfg = { baudRate: 4800, markFrequency: 9600, spaceFrequency: 14400 };
  const files = [new Uint8Array(0), Uint8Array.from({ length: 16 }, (_, i) => 255 - i), Uint8Array.from({ length: 75 }, (_, i) => (i * 37 + 1) & 0xff)];
  const nFrag = [1, 1, 5];
  const A = new P.FSKProcessorBatch(new M.FSKBatch(S, cfg), { clearRxOnTxComplete: true });
  const B = new P.FSKProcessorBatch(new M.FSKBatch(S, cfg), { clearRxOnTxComplete: true });
  const tx = new X.XModemSenderBatch(A, { maxPayloadSize });
  const rx = new X.XModemReceiverBatch(B);
  tx.send(files);
  assert.deepStrictEqual(Array.from(tx.state().state), [1, 1, 1]);
  assert.throws(() => tx.send(files, { mask: [0, 1, 0] }), /Transport busy: sendData cannot start while in SENDING_WAIT_NAK state \(stream 1\)/);
  assert.deepStrictEqual(tx.poll().streams.length, 0);   // nothing has arrived: empty replies
  B.modulate([[NAK], [NAK], [NAK]].map((x) => Uint8Array.from(x)));   // sendInitialNAK
  const got = files.map(() => []), owed = files.map(() => []), ended = {}, done = [false, false, false];
  let aOut = new Float32Array(S * Q), bOut = new Float32Array(S * Q);
  for (let q = 0; q < 4000 && Object.keys(ended).length < S; q++) {
    const aNext = A.process(bOut, Q, Q), bNext = B.process(aOut, Q, Q);
    aOut = aNext; bOut = bNext;
    if (q % 4 !== 3) continue;   // (both hosts act every fourth quantum: frames keep their distance)
    const t = tx.poll();
    t.streams.forEach((s, i) => { if (t.events[i].status !== 0) ended[s] = t.events[i].statusName; });
    const r = rx.poll({ mask: done.map((d) => !d) });
    r.streams.forEach((s, i) => {
      const res = r.results[i];
      got[s].push(...res.data);
      assert.ok(res.statusName === 'need_more' || res.statusName === 'eot', 'stream ' + s + ': ' + res.statusName);
      for (let k = 0; k < res.packets + res.dropped; k++) owed[s].push(ACK);
      if (res.statusName === 'eot') { owed[s].push(ACK); done[s] = true; }
    });
    const pending = B.txState().pending;
    const go = owed.map((o, s) => o.length > 0 && !pending[s]);
    if (go.some(Boolean)) B.modulate(go.map((g, s) => Uint8Array.from(g ? [owed[s].shift()] : [])), go);
  }
  assert.deepStrictEqual(ended, { 0: 'done', 1: 'done', 2: 'done' });
  files.forEach((f, s) => assert.deepStrictEqual(got[s], Array.from(f), 'stream ' + s));
  const st = tx.state();
  assert.deepStrictEqual(Array.from(st.state), [0, 0, 0]);
  assert.deepStrictEqual(Array.from(st.packetsSent), nFrag.map((n) => n + 1));   // the data packets and the EOT
  assert.deepStrictEqual(Array.from(st.retransmitted), [0, 0, 0]);
  assert.deepStrictEqual(Array.from(st.fragmentIndex), nFrag);
  assert.deepStrictEqual(Array.from(st.sequence), nFrag.map((n) => n + 1));
  assert.deepStrictEqual(Array.from(rx.state().packets), nFrag);
  // an abort ends a new transfer in its first wait; setState is validated by the library; reset drops everything
  tx.send(files);
  const ab = tx.poll({ abort: [0, 1, 0] });
  assert.deepStrictEqual([Array.from(ab.streams), ab.events[0].statusName, ab.events[0].error, ab.events[0].stateName], [[1], 'aborted', 'Operation aborted', 'IDLE']);
  assert.throws(() => tx.setState({ sequence: [1, 256, 1] }), /sequence\[1\] = 256 is not a sequence number/);
  tx.reset();
  assert.deepStrictEqual(Array.from(tx.state().packetsSent), [0, 0, 0]);
  tx.close();
  assert.throws(() => tx.poll(), /sender destroyed/);
  rx.close();
  for (const b of [A, B]) { b.close(); b.batch.close(); }
  console.log('js xmodem tx gpu tests ok');
}

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
