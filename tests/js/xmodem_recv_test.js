'use strict';
// XModemFileReceiverBatch through the N-API addon (include/fskhip_next.h: fskhip_xmodem_recv_*).
// cpu: the argument checks, which are made before the library is called, and the addon's own refusal of a handle that is none.
// gpu: three streams.  start() sends the initial NAK and a second start() throws the reference's busy text; a packet, an EOT and a packet
// with a bad CRC are planted into the receiver's rings (modulated on processor A, demodulated by processor B); ONE poll is then held to
// values computed here -- the events, the words, the files --, and files() / setFiles() round trip.
// usage: node xmodem_recv_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

function cpuTests() {
  for (const m of ['start', 'poll', 'files', 'setFiles', 'reset', 'state', 'setState', 'close']) assert.strictEqual(typeof X.XModemFileReceiverBatch.prototype[m], 'function');
  for (const f of ['Create', 'Destroy', 'Start', 'Poll', 'Reset', 'Files', 'SetFiles', 'State', 'SetState']) assert.strictEqual(typeof addon['xmodemRecv' + f], 'function');
  assert.throws(() => new X.XModemFileReceiverBatch(null), /processor must be an FSKProcessorBatch/);
  assert.throws(() => new X.XModemFileReceiverBatch({ nStreams: 4, handle: null }, null), /options must be an object/);
  for (const bad of [-1, 1.5, '16', 2 ** 32]) assert.throws(() => new X.XModemFileReceiverBatch({ nStreams: 4, handle: null }, { fileCapacity: bad }), /fileCapacity must be an integer/);
  for (const bad of [-1, 0.5, 2 ** 32]) assert.throws(() => new X.XModemFileReceiverBatch({ nStreams: 4, handle: null }, { maxRetries: bad }), /maxRetries must be an integer/);
  assert.throws(() => new X.XModemFileReceiverBatch({ nStreams: 4, handle: null }), /processor destroyed/);
  const b = Object.create(X.XModemFileReceiverBatch.prototype);   // no device here: the checks come before the handle is used
  b.nStreams = 4; b.handle = null;
  const files = [[1], [2], [], [3, 4]];
  assert.throws(() => b.start(null), /options must be an object/);
  assert.throws(() => b.start({ mask: 5 }), /mask must be an array/);
  assert.throws(() => b.start({ mask: [1, 0] }), /mask must have one entry per stream \(4\)/);
  assert.throws(() => b.poll(null), /options must be an object/);
  assert.throws(() => b.poll({ mask: 5 }), /mask must be an array/);
  assert.throws(() => b.poll({ timeout: 'yes' }), /timeout must be an array/);
  assert.throws(() => b.poll({ abort: [true] }), /abort must have one entry per stream \(4\)/);
  assert.throws(() => b.files(7), /streams must be an array/);
  assert.throws(() => b.files([0, 4]), /streams must hold integers in \[0, 4\)/);
  assert.throws(() => b.setFiles(7), /files must be an array/);
  assert.throws(() => b.setFiles([[1], [2]]), /files must have one entry per stream \(4\)/);
  assert.throws(() => b.setFiles(files, null), /options must be an object/);
  assert.throws(() => b.setFiles([[1], 'x', [], []]), /files\[1\] must be a byte array/);
  assert.throws(() => b.reset(1.5), /stream must be an integer/);
  assert.throws(() => b.setState(null), /state must be an object/);
  assert.throws(() => b.setState({ expected: 3 }), /expected must be an array/);
  assert.throws(() => b.setState({ fileLen: [1, 2] }), /fileLen must have one entry per stream \(4\)/);
  assert.throws(() => b.setState({ packetsSent: [1, 2, -1, 0] }), /packetsSent must hold integers/);
  // past the checks the calls reach the addon, which refuses what is no receiver handle
  assert.throws(() => b.start(), /receiver destroyed/);
  assert.throws(() => b.poll(), /receiver destroyed/);
  assert.throws(() => b.poll({ mask: [1, 0, 0, 1], timeout: [0, 1, 0, 0], abort: [0, 0, 1, 0] }), /receiver destroyed/);
  assert.throws(() => b.files(), /receiver destroyed/);
  assert.throws(() => b.files([3, 0]), /receiver destroyed/);
  assert.throws(() => b.setFiles(files), /receiver destroyed/);
  assert.throws(() => b.setFiles([null, [2], null, null], { mask: [0, 1, 0, 0] }), /receiver destroyed/);   // entries of unselected streams are not looked at
  assert.throws(() => b.reset(), /receiver destroyed/);
  assert.throws(() => b.state(), /receiver destroyed/);
  assert.throws(() => b.setState({ state: [0, 0, 0, 0] }), /receiver destroyed/);
  assert.throws(() => addon.xmodemRecvPoll(), /too few arguments/);
  b.close();   // nothing to close
  console.log('js xmodem recv cpu tests ok');
}

function crc16(data) {   // CRC-16-CCITT, 0x1021, initial 0xFFFF
  let c = 0xFFFF;
  for (const b of data) { c ^= b << 8; for (let k = 0; k < 8; k++) c = (c & 0x8000) ? ((c << 1) ^ 0x1021) & 0xFFFF : (c << 1) & 0xFFFF; }
  return c;
}

function gpuTests() {
  const S = 3, Q = 512, ACK = 0x06, NAK = 0x15, EOT = 0x04;
  const cfg = { baudRate: 4800, markFrequency: 9600, spaceFrequency: 14400 };
  const payload = Uint8Array.from({ length: 16 }, (_, i) => (i * 29 + 7) & 0xff);
  const crc = crc16(payload);
  const good = Uint8Array.from([0x01, 1, 254, 16, ...payload, crc >> 8, crc & 0xff]);
  const bad = Uint8Array.from([0x41, 0x01, 1, 254, 16, ...payload, crc >> 8, (crc & 0xff) ^ 0x20]);   // a noise byte, then a packet whose CRC is off
  const A = new P.FSKProcessorBatch(new M.FSKBatch(S, cfg), { clearRxOnTxComplete: false });
  const B = new P.FSKProcessorBatch(new M.FSKBatch(S, cfg), { clearRxOnTxComplete: false });
  const rx = new X.XModemFileReceiverBatch(B, { fileCapacity: 64, maxRetries: 3 });
  rx.start();
  assert.deepStrictEqual(Array.from(rx.state().state), [1, 1, 1]);
  assert.deepStrictEqual(Array.from(rx.state().packetsSent), [1, 1, 1]);
  assert.throws(() => rx.start({ mask: [0, 1, 0] }), /Transport busy: receiveData cannot start while in RECEIVING_SEND_NAK state \(stream 1\)/);
  assert.deepStrictEqual(Array.from(B.txState().pending, Boolean), [true, true, true]);   // the initial NAK is on its way
  assert.strictEqual(rx.poll().streams.length, 0);                             // mid-modulation: nothing happens
  assert.deepStrictEqual(Array.from(rx.state().state), [1, 1, 1]);
  // plant the rings: A modulates, B demodulates
  A.modulate([good, Uint8Array.from([EOT]), bad]);
  let aOut = new Float32Array(S * Q), bOut = new Float32Array(S * Q);
  for (let q = 0; q < 40; q++) {
    const aNext = A.process(bOut, Q, Q), bNext = B.process(aOut, Q, Q);
    aOut = aNext; bOut = bNext;
  }
  assert.deepStrictEqual(Array.from(B.txState().pending, Boolean), [false, false, false]);
  const r = rx.poll({ timeout: [1, 0, 0] });   // (a timeout flag on a stream with a complete packet is ignored)
  assert.deepStrictEqual(Array.from(r.streams), [0, 1, 2]);
  const pick = (e) => [e.statusName, e.error, e.stateName, e.control, e.stepName, e.seq, e.len, e.acceptedLen, e.fileLen, e.expected, e.retries, e.crcRx, e.crcCalc];
  assert.deepStrictEqual(pick(r.events[0]), ['progress', null, 'RECEIVING_SEND_ACK', ACK, 'need_more', 1, 16, 16, 16, 2, 0, -1, -1]);
  assert.deepStrictEqual(pick(r.events[1]), ['done', null, 'IDLE', ACK, 'eot', -1, -1, 0, 0, 1, 0, -1, -1]);
  assert.deepStrictEqual(pick(r.events[2]), ['progress', null, 'RECEIVING_WAIT_BLOCK', NAK, 'invalid_crc', 1, 16, 0, 0, 1, 1, crc ^ 0x20, crc]);
  const st = rx.state();
  assert.deepStrictEqual(RECV_WORDS.map((k) => Array.from(st[k])), [[3, 0, 2], [2, 1, 1], [0, 0, 1], [16, 0, 0], [1, 0, 1], [0, 0, 1], [2, 2, 2]]);
  assert.deepStrictEqual(Array.from(B.txState().pending, Boolean), [true, true, true]);   // the replies are being modulated
  assert.deepStrictEqual(Array.from(B.rxLengths()), [0, 0, 0]);
  // files(): what arrived; setFiles() puts files back, files() returns them
  assert.deepStrictEqual(rx.files().map((f) => Array.from(f)), [Array.from(payload), [], []]);
  assert.deepStrictEqual(rx.files([2, 0]).map((f) => f.length), [0, 16]);
  const back = [Uint8Array.from({ length: 64 }, (_, i) => 255 - i), null, Uint8Array.from([9, 8, 7])];
  rx.setFiles(back, { mask: [1, 0, 1] });
  assert.deepStrictEqual(rx.files().map((f) => Array.from(f)), [Array.from(back[0]), [], [9, 8, 7]]);
  assert.deepStrictEqual(Array.from(rx.state().fileLen), [64, 0, 3]);
  assert.throws(() => rx.setFiles([new Uint8Array(65), null, null], { mask: [1, 0, 0] }), /file_capacity is 64/);
  assert.throws(() => rx.setState({ expected: [1, 256, 1] }), /expected\[1\] = 256 is not a sequence number/);
  // an abort ends a transfer; reset drops everything
  const ab = rx.poll({ abort: [0, 0, 1] });
  assert.deepStrictEqual([Array.from(ab.streams), ab.events[0].statusName, ab.events[0].error, ab.events[0].stateName], [[2], 'aborted', 'Operation aborted', 'IDLE']);
  rx.reset();
  assert.deepStrictEqual(RECV_WORDS.map((k) => Array.from(rx.state()[k])), [[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]);
  rx.close();
  assert.throws(() => rx.poll(), /receiver destroyed/);
  for (const b of [A, B]) { b.close(); b.batch.close(); }
  console.log('js xmodem recv gpu tests ok');
}
const RECV_WORDS = ['state', 'expected', 'retries', 'fileLen', 'packetsReceived', 'dropped', 'packetsSent'];

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
