'use strict';
// XModemTimers.remap / snapshot / fromSnapshot and xmodemTimerSnapshotInfo through the N-API addon (include/fskhip_next.h:
// fskhip_xmodem_timer_remap, _snapshot, _restore, _snapshot_info_get).
// cpu: the surface, the image validator on images built here from the documented format, the kind-mismatch TypeError's way in.
// gpu: random valid words set with setState at 70 streams reach the destination as the take by the map says, 0 and 0 at -1, through
// remap and through snapshot / fromSnapshot, for both kinds and the map shapes of tests/test_gpu_xmodem_timer_remap.py; the image's
// bytes; xmodemTimerSnapshotInfo; the kind-mismatch TypeError; a destination that is no longer fresh.
// usage: node xmodem_timer_remap_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

const MASK = (1n << 64n) - 1n;
// the processor snapshot's checksum over the image's u64 words, the checksum field taken as 0
function checksum(buf) {
  let a = 0n, b = 0n;
  for (let i = 0; i + 8 <= buf.length; i += 8) { a = (a + (i === 32 ? 0n : buf.readBigUInt64LE(i))) & MASK; b = (b + a) & MASK; }
  return ((a * 0x9E3779B97F4A7C15n) & MASK) ^ b;
}
// an image from the documented format: header 48 bytes, (waited, mark) per record, zeros to 16
function image(kind, records, timeout, over = {}) {
  const size = (48 + 8 * records.length + 15) & ~15;
  const buf = Buffer.alloc(size);
  [over.magic === undefined ? 0x574B5346 : over.magic, 1, 48, kind, records.length, 2, timeout, 0].forEach((v, i) => buf.writeUInt32LE(v, 4 * i));
  records.forEach(([w, m], r) => { buf.writeUInt32LE(w, 48 + 8 * r); buf.writeUInt32LE(m, 52 + 8 * r); });
  buf.writeBigUInt64LE(checksum(buf), 32);
  return buf;
}

function cpuTests() {
  for (const m of ['remap', 'snapshot']) assert.strictEqual(typeof X.XModemTimers.prototype[m], 'function');
  assert.strictEqual(typeof X.XModemTimers.fromSnapshot, 'function');
  assert.strictEqual(typeof X.xmodemTimerSnapshotInfo, 'function');
  for (const f of ['Remap', 'Snapshot', 'Restore', 'SnapshotInfo']) assert.strictEqual(typeof addon['xmodemTimer' + f], 'function');
  const good = image(3, [[0, 0], [12287, 2], [0xffffffff, 5]], 12288);
  assert.deepStrictEqual(X.xmodemTimerSnapshotInfo(good), { kind: 3, nStreams: 3, timeoutSamples: 12288 });
  assert.deepStrictEqual(X.xmodemTimerSnapshotInfo(image(2, [], 1)), { kind: 2, nStreams: 0, timeoutSamples: 1 });
  assert.throws(() => X.xmodemTimerSnapshotInfo(image(3, [[1, 8]], 5)), /record 0: mark 8 is not a mark/);
  assert.throws(() => X.xmodemTimerSnapshotInfo(image(2, [[1, 1]], 5)), /mark 1 has a stage, a sender's timer has none/);
  assert.throws(() => X.xmodemTimerSnapshotInfo(image(3, [[1, 0]], 5, { magic: 0x584B5346 })), /is an XModem handle's snapshot's/);
  assert.throws(() => X.xmodemTimerSnapshotInfo(good.subarray(0, 56)), /do not match the layout/);
  const bad = Buffer.from(good); bad[50] ^= 1;
  assert.throws(() => X.xmodemTimerSnapshotInfo(bad), /a damaged snapshot/);
  // the image is validated before the handle is looked at; a closed object refuses before the library is called
  const rx = Object.create(X.XModemFileReceiverBatch.prototype);
  rx.nStreams = 3; rx.handle = null;
  assert.throws(() => X.XModemTimers.fromSnapshot(rx, bad), /a damaged snapshot/);
  assert.throws(() => X.XModemTimers.fromSnapshot(rx, good), /the handle has been closed/);
  const t = Object.create(X.XModemTimers.prototype);
  t.nStreams = 3; t.recv = true; t.over = rx; t.handle = null; t.timeoutSamples = 7;
  assert.throws(() => t.remap(rx, [0, 1, 2]), /remap: the timers have been closed/);
  assert.throws(() => t.snapshot(), /snapshot: the timers have been closed/);
  console.log('js xmodem timer remap cpu tests ok');
}

const S = 70;
const cfg = { baudRate: 1200, markFrequency: 1200, spaceFrequency: 2200 };
const TIMEOUT = { recv: 12288, tx: 8192 }, MARKS = { recv: [0, 1, 2, 4, 5, 6], tx: [0, 4] }, KIND = { tx: 2, recv: 3 };

let seed = 0x71A0;
const rnd = (n) => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return Math.floor(seed / 2 ** 32 * n); };

function gpuTests() {
  const made = [];
  const stack = (kind, n) => {
    const p = new P.FSKProcessorBatch(new M.FSKBatch(n, cfg), { rxCapacity: 1024 });
    const h = kind === 'recv' ? new X.XModemFileReceiverBatch(p, { fileCapacity: 64 }) : new X.XModemSenderBatch(p, { maxPayloadSize: 16 });
    made.push({ p, h });
    return h;
  };
  const words = (kind, n) => {
    const edge = [0, 1, TIMEOUT[kind] - 1, TIMEOUT[kind], 0xffffffff];
    return { waited: Uint32Array.from({ length: n }, (_, s) => (s < edge.length ? edge[s] : rnd(2 ** 32))),
      mark: Uint32Array.from({ length: n }, (_, s) => MARKS[kind][s < MARKS[kind].length ? s : rnd(MARKS[kind].length)]) };
  };
  const take = (w, map) => ({ waited: map.map((m) => (m < 0 ? 0 : w.waited[m])), mark: map.map((m) => (m < 0 ? 0 : w.mark[m])) });
  const plain = (st) => ({ waited: Array.from(st.waited), mark: Array.from(st.mark) });
  const ident = Array.from({ length: S }, (_, i) => i);
  const shuffled = (a) => { const b = a.slice(); for (let i = b.length - 1; i > 0; i--) { const j = rnd(i + 1); [b[i], b[j]] = [b[j], b[i]]; } return b; };
  const maps = {
    shrink: shuffled(ident).slice(0, 50).sort((x, y) => x - y),
    grow: shuffled(ident.concat(Array(14).fill(-1))),
    clones: ident.map(() => rnd(S)),
    'all-new': Array(S).fill(-1),
    'identity-but-one': ident.map((i) => (i === 41 ? -1 : i)),
  };
  const images = {};
  for (const kind of ['recv', 'tx']) {
    const src = new X.XModemTimers(stack(kind, S), { timeoutSamples: TIMEOUT[kind] });
    const w = words(kind, S);
    src.setState(w);
    for (const [name, map] of Object.entries(maps)) {
      const dst = stack(kind, map.length), want = take(w, map);
      const a = src.remap(dst, map);
      const b = X.XModemTimers.fromSnapshot(dst, src.snapshot(), map);
      assert.deepStrictEqual([a.nStreams, a.timeoutSamples, b.nStreams, b.timeoutSamples], [map.length, TIMEOUT[kind], map.length, TIMEOUT[kind]], name);
      assert.deepStrictEqual(plain(a.state()), want, kind + ' remap ' + name);
      assert.deepStrictEqual(plain(b.state()), want, kind + ' fromSnapshot ' + name);
      const img = a.snapshot();
      assert.ok(img.equals(b.snapshot()) && img.equals(image(KIND[kind], map.map((m, i) => [want.waited[i], want.mark[i]]), TIMEOUT[kind])), kind + ' image ' + name);
      assert.deepStrictEqual(X.xmodemTimerSnapshotInfo(img), { kind: KIND[kind], nStreams: map.length, timeoutSamples: TIMEOUT[kind] });
      if (!map.includes(-1)) assert.ok(img.equals(src.snapshot(map)), kind + ' selection ' + name);
      a.close(); b.close();
    }
    assert.deepStrictEqual(plain(src.state()), plain(w));   // the source is read only
    // the timeout: the source's, the image's, or the caller's
    const dst = stack(kind, S);
    const c = src.remap(dst, ident, { timeoutSamples: 999 }), d = X.XModemTimers.fromSnapshot(dst, src.snapshot(), null, { timeoutSamples: 777 });
    assert.deepStrictEqual([c.timeoutSamples, d.timeoutSamples, X.xmodemTimerSnapshotInfo(d.snapshot()).timeoutSamples], [999, 777, 777]);
    assert.deepStrictEqual(plain(d.state()), plain(w));
    // a destination that is no longer fresh is refused and left as it was
    d.reset(0);
    const held = plain(d.state());
    assert.throws(() => addon.xmodemTimerRemap(d.handle, src.handle, ident), /used already/);
    assert.throws(() => addon.xmodemTimerRestore(d.handle, src.snapshot(), ident), /used already/);
    assert.deepStrictEqual(plain(d.state()), held);
    // a second remap into a still-fresh one replaces the first
    addon.xmodemTimerRemap(c.handle, src.handle, maps.clones);
    assert.deepStrictEqual(plain(c.state()), take(w, maps.clones));
    assert.throws(() => addon.xmodemTimerRemap(c.handle, src.handle, ident.slice(1)), /n_map 69 != the destination's 70 streams/);
    assert.throws(() => addon.xmodemTimerRemap(c.handle, src.handle, ident.map((i) => (i === 3 ? S : i))), /map\[3\] = 70, the source has 70 streams/);
    assert.deepStrictEqual(plain(c.state()), take(w, maps.clones));
    images[kind] = src.snapshot();
    for (const t of [c, d, src]) t.close();
  }
  // the kind mismatch: a TypeError that names both kinds, and the library's own refusal
  const recvH = stack('recv', S), txH = stack('tx', S);
  assert.throws(() => X.XModemTimers.fromSnapshot(recvH, images.tx), (e) => e instanceof TypeError && /the snapshot is of kind 'tx', the handle's is 'recv'/.test(e.message));
  assert.throws(() => X.XModemTimers.fromSnapshot(txH, images.recv), (e) => e instanceof TypeError && /the snapshot is of kind 'recv', the handle's is 'tx'/.test(e.message));
  const r = new X.XModemTimers(recvH, { timeoutSamples: 5 }), t = new X.XModemTimers(txH, { timeoutSamples: 5 });
  assert.throws(() => addon.xmodemTimerRemap(r.handle, t.handle, ident), /different kinds/);
  assert.throws(() => addon.xmodemTimerRestore(t.handle, images.recv, ident), /the snapshot is of kind 3 \(recv\), this timer's is 2 \(tx\)/);
  assert.throws(() => r.remap(txH, ident), /different kinds/);
  r.close(); t.close();
  for (const { p, h } of made) { h.close(); p.close(); p.batch.close(); }
  console.log('js xmodem timer remap gpu tests ok');
}

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
