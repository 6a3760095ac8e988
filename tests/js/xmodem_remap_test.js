'use strict';
// remap / snapshot / fromSnapshot of the three resident XModem classes through the N-API addon (include/fskhip_next.h:
// fskhip_xmodem_{rx,tx,recv}_remap / _snapshot / _restore, fskhip_xmodem_snapshot_info_get).
// cpu: the surface, and the refusals that need no device.
// gpu: 70 streams per class, state and files from the formulas tests/test_node_xmodem_remap.py uses; the remapped object's image and the
// image of a snapshot round trip under the same map are hashed and held to the digests the Python binding got (argv[3..5]).
// usage: node xmodem_remap_test.js cpu | gpu <rx digest> <tx digest> <recv digest>
const assert = require('assert');
const crypto = require('crypto');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

const CLASSES = { rx: X.XModemReceiverBatch, tx: X.XModemSenderBatch, recv: X.XModemFileReceiverBatch };

function cpuTests() {
  for (const C of Object.values(CLASSES)) {
    assert.strictEqual(typeof C.prototype.remap, 'function');
    assert.strictEqual(typeof C.prototype.snapshot, 'function');
    assert.strictEqual(typeof C.fromSnapshot, 'function');
  }
  assert.strictEqual(typeof X.xmodemSnapshotInfo, 'function');
  for (const k of ['Rx', 'Tx', 'Recv']) for (const f of ['Remap', 'Snapshot', 'Restore']) assert.strictEqual(typeof addon['xmodem' + k + f], 'function');
  // an empty image of each kind, made here from the documented layout: 48 bytes, the checksum over its six words
  const image = (kind, words, p0, p1) => {
    const b = Buffer.alloc(48);
    [0x584B5346, 1, 48, kind, 0, words, p0, p1].forEach((v, i) => b.writeUInt32LE(v, 4 * i));
    let a = 0n, s = 0n;
    const mask = (1n << 64n) - 1n;
    for (let i = 0; i < 48; i += 8) { a = (a + b.readBigUInt64LE(i)) & mask; s = (s + a) & mask; }
    b.writeBigUInt64LE(((a * 0x9E3779B97F4A7C15n) & mask) ^ s, 32);
    return b;
  };
  assert.deepStrictEqual(X.xmodemSnapshotInfo(image(2, 8, 128, 10)), { kind: 2, nStreams: 0, param0: 128, param1: 10, fileBytes: 0 });
  assert.deepStrictEqual(X.xmodemSnapshotInfo(image(3, 8, 600, 3)), { kind: 3, nStreams: 0, param0: 600, param1: 3, fileBytes: 0 });
  assert.deepStrictEqual(X.xmodemSnapshotInfo(image(1, 4, 0, 0)), { kind: 1, nStreams: 0, param0: 0, param1: 0, fileBytes: 0 });
  const bad = image(2, 8, 128, 10);
  bad[28] ^= 1;
  assert.throws(() => X.xmodemSnapshotInfo(bad), /checksum/);
  assert.throws(() => X.xmodemSnapshotInfo(image(2, 4, 128, 10)), /record_words 4/);
  assert.throws(() => X.XModemSenderBatch.fromSnapshot({ nStreams: 0, handle: null }, image(1, 4, 0, 0)), /the snapshot is of kind 'rx', not 'tx'/);
  assert.throws(() => addon.xmodemRecvRestore(null, image(2, 8, 128, 10), []), /the snapshot is of kind 2 \(tx\), this handle's is 3 \(recv\)/);
  assert.throws(() => addon.xmodemTxRestore(null, image(2, 8, 128, 10), [0]), /map\[0\] = 0, the snapshot has 0 records/);
  assert.throws(() => addon.xmodemTxRestore(null, image(2, 8, 128, 10), []), /null handle/);
  assert.throws(() => addon.xmodemRxRemap(null, null, []), /destroyed/);
  console.log('js xmodem remap cpu tests ok');
}

// the formulas of tests/test_node_xmodem_remap.py
const S = 70;
const LENGTHS = [0, 1, 15, 16, 17, 127, 128, 129, 600];
const fileOf = (s) => Uint8Array.from({ length: LENGTHS[s % 9] }, (_, k) => (s * 31 + k * 7 + 1) & 0xff);
const MAP = Array.from({ length: 64 }, (_, i) => (i % 9 === 4 ? -1 : (i * 37 + 11) % S));
const u32 = (f) => Uint32Array.from({ length: S }, (_, s) => f(s));

function gpuTests(want) {
  const batch = (n) => new P.FSKProcessorBatch(new M.FSKBatch(n, {}), { rxCapacity: 300 });
  const sha = (b) => crypto.createHash('sha256').update(b).digest('hex');
  const make = {
    rx: (p) => {
      const h = new X.XModemReceiverBatch(p);
      h.setState({ expected: u32((s) => 1 + (s * 13) % 255), packets: u32((s) => s * 3), dropped: u32((s) => s % 7) });
      return h;
    },
    tx: (p) => {
      const h = new X.XModemSenderBatch(p, { maxPayloadSize: 128, maxRetries: 3 });
      const has = Array.from({ length: S }, (_, s) => s % 5 !== 0);
      h.send(Array.from({ length: S }, (_, s) => fileOf(s)), { mask: has });
      const frags = (s) => Math.max(1, Math.ceil(LENGTHS[s % 9] / 128));
      h.setState({ state: u32((s) => (has[s] ? s % 4 : 0)), sequence: u32((s) => 1 + (s * 17) % 255),
        fragmentIndex: u32((s) => (has[s] && (s % 4 === 1 || s % 4 === 2) ? s % frags(s) : 0)), retries: u32((s) => s % 3), packetsSent: u32((s) => s * 5),
        retransmitted: u32((s) => s % 11) });
      return h;
    },
    recv: (p) => {
      const h = new X.XModemFileReceiverBatch(p, { fileCapacity: 600, maxRetries: 3 });
      h.setFiles(Array.from({ length: S }, (_, s) => fileOf(s + 3)));
      h.setState({ state: u32((s) => s % 4), expected: u32((s) => 1 + (s * 19) % 255), retries: u32((s) => s % 4), packetsReceived: u32((s) => s * 2),
        dropped: u32((s) => s % 5), packetsSent: u32((s) => s + 1) });
      return h;
    },
  };
  for (const kind of ['rx', 'tx', 'recv']) {
    const src = batch(S), h = make[kind](src);
    const dst = batch(MAP.length), next = h.remap(dst, MAP);
    assert.strictEqual(next.nStreams, MAP.length);
    const image = next.snapshot();
    const info = X.xmodemSnapshotInfo(image);
    assert.strictEqual(info.nStreams, MAP.length);
    assert.strictEqual(info.kind, { rx: 1, tx: 2, recv: 3 }[kind]);
    assert.strictEqual(sha(image), want[kind], kind + ': the remapped image differs from the Python binding\'s');
    // the snapshot round trip lands in the same place, and the source is as it was
    const whole = h.snapshot();
    const dst2 = batch(MAP.length), back = CLASSES[kind].fromSnapshot(dst2, whole, MAP);
    assert.strictEqual(sha(back.snapshot()), want[kind], kind + ': the restored image differs');
    assert.ok(whole.equals(h.snapshot()));
    assert.ok(h.snapshot(MAP.filter((m) => m >= 0)).equals(next.snapshot(MAP.map((m, i) => (m >= 0 ? i : -1)).filter((i) => i >= 0))));
    for (const x of [next, back, h]) x.close();
    for (const p of [dst, dst2, src]) { p.close(); p.batch.close(); }
  }
  console.log('js xmodem remap gpu tests ok');
}

if (process.argv[2] === 'cpu') cpuTests();
else if (process.argv[2] === 'gpu') gpuTests({ rx: process.argv[3], tx: process.argv[4], recv: process.argv[5] });
else { console.error('usage: node xmodem_remap_test.js cpu|gpu <rx> <tx> <recv>'); process.exit(2); }
