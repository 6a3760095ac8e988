'use strict';
// XModemTimers through the N-API addon (include/fskhip_next.h: fskhip_xmodem_timer_*, fskhip_xmodem_*_poll_timed_host).
// cpu: the argument checks, which are made before the library is called, and the addon's own refusal of a handle that is none.
// gpu: the twin of tests/test_gpu_xmodem_timer.py at 70 streams, Bell 202 at 1 200 baud, quanta of 128: two identical processor /
// handle pairs hear the same line (a third processor whose modulator plays the scripted bytes); one pair is polled through
// XModemTimers.poll, the other through the plain poll with the masks of a model of the contract written here.  After every quantum the
// lists, the events, the handle's words, the timers' words, the ring lengths and the transmit state must be equal.
// usage: node xmodem_timer_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const X = require(path.join(__dirname, '..', '..', 'napi', 'xmodem.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

function cpuTests() {
  for (const m of ['poll', 'reset', 'state', 'setState', 'close']) assert.strictEqual(typeof X.XModemTimers.prototype[m], 'function');
  for (const f of ['Create', 'Destroy', 'Poll', 'Reset', 'State', 'SetState']) assert.strictEqual(typeof addon['xmodemTimer' + f], 'function');
  assert.throws(() => new X.XModemTimers(null), /handle must be an XModemFileReceiverBatch or an XModemSenderBatch/);
  assert.throws(() => new X.XModemTimers({ nStreams: 4, handle: 1 }), /handle must be an XModemFileReceiverBatch or an XModemSenderBatch/);
  const rx = Object.create(X.XModemFileReceiverBatch.prototype);   // no device here: the checks come before the handle is used
  rx.nStreams = 4; rx.handle = null;
  assert.throws(() => new X.XModemTimers(rx), /the handle has been closed/);
  rx.handle = {};   // not a receiver handle: the addon refuses it, after the checks
  assert.throws(() => new X.XModemTimers(rx, null), /options must be an object/);
  for (const bad of [0, -1, 1.5, '9', 2 ** 32]) assert.throws(() => new X.XModemTimers(rx, { timeoutSamples: bad }), /the timeout must be an integer number of samples/);
  assert.throws(() => new X.XModemTimers(rx, { timeoutMs: 0 }), /the timeout must be an integer number of samples/);
  assert.throws(() => new X.XModemTimers(rx), /receiver destroyed/);
  assert.throws(() => new X.XModemTimers(rx, { timeoutMs: 3000 }), /receiver destroyed/);
  const t = Object.create(X.XModemTimers.prototype);
  t.nStreams = 4; t.recv = true; t.over = rx; t.handle = null;
  assert.throws(() => t.poll(128), /the timers have been closed/);
  t.handle = {};
  assert.throws(() => t.poll(-1), /elapsed must be an integer number of samples/);
  assert.throws(() => t.poll(1.5), /elapsed must be an integer number of samples/);
  assert.throws(() => t.poll(128, null), /options must be an object/);
  assert.throws(() => t.poll(128, { mask: 5 }), /mask must be an array/);
  assert.throws(() => t.poll(128, { abort: [true] }), /abort must have one entry per stream \(4\)/);
  assert.throws(() => t.reset(1.5), /stream must be an integer/);
  assert.throws(() => t.setState(null), /state must be an object/);
  assert.throws(() => t.setState({ waited: 3 }), /waited must be an array/);
  assert.throws(() => t.setState({ mark: [1, 2] }), /mark must have one entry per stream \(4\)/);
  assert.throws(() => t.poll(128), /timers destroyed/);
  assert.throws(() => t.poll(128, { mask: [1, 0, 0, 1], abort: [0, 0, 1, 0] }), /timers destroyed/);
  assert.throws(() => t.reset(), /timers destroyed/);
  assert.throws(() => t.state(), /timers destroyed/);
  assert.throws(() => t.setState({ waited: [0, 0, 0, 0] }), /timers destroyed/);
  rx.handle = null;
  assert.throws(() => t.poll(128), /the timers' handle has been closed/);
  assert.throws(() => addon.xmodemTimerPoll(), /too few arguments/);
  t.handle = null;
  t.close();   // nothing to close
  console.log('js xmodem timer cpu tests ok');
}

function crc16(data) {   // CRC-16-CCITT, 0x1021, initial 0xFFFF
  let c = 0xFFFF;
  for (const b of data) { c ^= b << 8; for (let k = 0; k < 8; k++) c = (c & 0x8000) ? ((c << 1) ^ 0x1021) & 0xFFFF : (c << 1) & 0xFFFF; }
  return c;
}

const S = 70, Q = 128, SOH = 0x01, EOT = 0x04, ACK = 0x06, NAK = 0x15;
const cfg = { baudRate: 1200, markFrequency: 1200, spaceFrequency: 2200 };

// the contract's fire and arm, per stream
class Model {
  constructor(timeout, recv) { this.waited = new Uint32Array(S); this.mark = new Uint32Array(S); this.timeout = timeout; this.recv = recv; }
  fire(elapsed, mask, state, pending, held) {
    this.kind = new Uint8Array(S); this.held = Uint32Array.from(held);
    const flag = new Uint8Array(S);
    for (let s = 0; s < S; s++) {
      if (state[s] === 0 || !mask[s]) continue;
      if (pending[s]) { this.kind[s] = 1; this.mark[s] |= 4; continue; }
      this.kind[s] = 2;
      if ((this.mark[s] & 4) || (this.recv && (state[s] === 1 || state[s] === 3))) { this.waited[s] = 0; this.mark[s] = 0; } else this.waited[s] = Math.min(this.waited[s] + elapsed, 0xffffffff);
      flag[s] = this.waited[s] >= this.timeout ? 1 : 0;
    }
    return flag;
  }
  arm(polled, stateAfter, live) {
    const ev = new Map(Array.from(polled.streams, (s, i) => [s, polled.events[i]]));
    for (let s = 0; s < S; s++) {
      if (!this.kind[s]) continue;
      if (stateAfter[s] === 0) { this.waited[s] = 0; this.mark[s] = 0; continue; }
      if (this.kind[s] !== 2) continue;
      const e = ev.get(s);
      if (this.recv) {
        const stage = live[s] === 0 ? 0 : live[s] < 4 ? 1 : 2;
        if (e || live[s] < this.held[s] || stage > (this.mark[s] & 3)) this.waited[s] = 0;
        this.mark[s] = (this.mark[s] & ~3) | stage;
      } else if (e && (e.sentLen !== 0 || e.status !== 0 || (e.stateAfter === 2 && e.control === EOT))) this.waited[s] = 0;
    }
  }
}

function twins(recv, timeout, nQuanta, make, mask, aborts, script) {
  const mk = () => new P.FSKProcessorBatch(new M.FSKBatch(S, cfg), { rxCapacity: 1024 });
  const line = mk(), A = mk(), B = mk();
  const ha = make(A), hb = make(B);
  const timers = new X.XModemTimers(ha, { timeoutSamples: timeout });
  const model = new Model(timeout, recv);
  const seen = Array.from({ length: S }, () => []), when = Array.from({ length: S }, () => []);
  const silence = new Float32Array(S * Q);
  const plain = (o) => JSON.stringify(o, (k, v) => (ArrayBuffer.isView(v) ? Array.from(v) : v));
  const play = (rows) => {   // rows: Map stream -> bytes, started on the line now
    if (rows.size) line.modulate(Array.from({ length: S }, (_, s) => rows.get(s) || new Uint8Array(0)), Array.from({ length: S }, (_, s) => rows.has(s)));
  };
  for (let q = 0; q < nQuanta; q++) {
    play(script(q, null));
    const x = line.process(silence, Q, Q);
    A.process(x, Q, Q);
    B.process(x, Q, Q);
    const abort = aborts.get(q) || null;
    const pa = timers.poll(Q, { mask, abort });
    const flag = model.fire(Q, mask, hb.state().state, B.txState().pending, B.rxLengths());
    const pb = recv ? hb.poll({ mask, timeout: flag, abort }) : hb.poll({ mask, abort: abort ? flag.map((f, s) => f | abort[s]) : flag });
    model.arm(pb, hb.state().state, B.rxLengths());
    assert.strictEqual(plain(pa), plain(pb), 'events, quantum ' + q);
    assert.strictEqual(plain([ha.state(), A.rxLengths(), A.txState()]), plain([hb.state(), B.rxLengths(), B.txState()]), 'words, quantum ' + q);
    assert.strictEqual(plain(timers.state()), plain({ waited: model.waited, mark: model.mark }), 'timers, quantum ' + q);
    Array.from(pa.streams).forEach((s, i) => { seen[s].push(pa.events[i]); when[s].push(q); });
    play(script(q, pa));
  }
  const out = { seen, when, state: ha.state(), timers: timers.state() };
  timers.close();
  assert.throws(() => timers.poll(Q), /the timers have been closed/);
  for (const h of [ha, hb]) h.close();
  for (const b of [line, A, B]) { b.close(); b.batch.close(); }
  return out;
}

function gpuTests() {
  const kind = (s) => s % 5;
  const mask = Array.from({ length: S }, (_, s) => kind(s) !== 2);
  const payload = Uint8Array.from([0x61, 0x62]);
  const crc = crc16(payload);
  const p1 = Uint8Array.from([SOH, 1, 254, 2, ...payload, crc >> 8, crc & 0xff]);
  const rows = (pick) => { const m = new Map(); for (let s = 0; s < S; s++) { const r = pick(s); if (r) m.set(s, r); } return m; };
  // the file receiver.  by stream % 5: 0 hears nothing; 1 hears noise; 2 is masked out; 3 a whole packet, then EOT; 4 is aborted by the caller
  const timeout = 4096;
  let r = twins(true, timeout, 170, (p) => { const h = new X.XModemFileReceiverBatch(p, { fileCapacity: 64, maxRetries: 2 }); h.start(); return h; }, mask,
    new Map([[30, Array.from({ length: S }, (_, s) => kind(s) === 4)]]),
    (q, polled) => {
      if (polled) return new Map();
      if (q === 16) return rows((s) => (kind(s) === 1 ? Uint8Array.from([0x33, 0x77]) : null));
      if (q === 20) return rows((s) => (kind(s) === 3 ? p1 : null));
      if (q === 70) return rows((s) => (kind(s) === 3 ? Uint8Array.from([EOT]) : null));
      return new Map();
    });
  for (let s = 0; s < S; s++) {
    const ev = r.seen[s];
    if (kind(s) === 0) assert.deepStrictEqual(ev.map((e) => [e.statusName, e.control]), [['progress', NAK], ['progress', NAK], ['max_retries', -1]]);
    else if (kind(s) === 1) assert.ok(ev[0].control === NAK && r.when[s][0] > r.when[0][0]);   // the noise re-armed the timer
    else if (kind(s) === 2) assert.ok(ev.length === 0 && r.state.state[s] === 1 && r.timers.waited[s] === 0 && r.timers.mark[s] === 0);
    else if (kind(s) === 3) assert.deepStrictEqual(ev.slice(0, 2).map((e) => [e.statusName, e.control, e.fileLen]), [['progress', ACK, 2], ['done', ACK, 2]]);
    else assert.deepStrictEqual(ev.map((e) => e.statusName), ['aborted']);
  }
  // the sender.  by stream % 5: 0 hears nothing; 1 bytes that are no control bytes (aborted at the same poll as 0); 2 is masked out; 3 runs a whole
  // transfer of two fragments; 4 a NAK, then an EOT while it waits for the ACK (re-armed), then nothing
  const after = (sentLen) => Math.ceil((sentLen + 3) * 400 / Q) + 3;
  const due = new Map();   // quantum -> Map stream -> bytes
  const at = (q, s, bytes) => { if (!due.has(q)) due.set(q, new Map()); due.get(q).set(s, bytes); };
  r = twins(false, 3072, 175, (p) => { const h = new X.XModemSenderBatch(p, { maxPayloadSize: 4, maxRetries: 2 }); h.send(Array.from({ length: S }, () => Uint8Array.from([1, 2, 3, 4, 5, 6]))); return h; },
    mask, new Map(), (q, polled) => {
      if (!polled) {
        const now = due.get(q) || new Map();
        if (q === 2) for (let s = 0; s < S; s++) { if (kind(s) === 1) now.set(s, Uint8Array.from([0x78, 0x79])); else if (kind(s) >= 3) now.set(s, Uint8Array.from([NAK])); }
        return now;
      }
      Array.from(polled.streams).forEach((s, i) => {
        const e = polled.events[i];
        if (!e.sentLen) return;
        if (kind(s) === 3) at(q + after(e.sentLen), s, Uint8Array.from([ACK]));
        else if (kind(s) === 4) at(q + after(e.sentLen) + 6, s, Uint8Array.from([EOT]));
      });
      return new Map();
    });
  for (let s = 0; s < S; s++) {
    const ev = r.seen[s].map((e) => [e.statusName, e.control]);
    if (kind(s) <= 1) { assert.deepStrictEqual(ev, [['aborted', -1]]); assert.strictEqual(r.when[s][0], 3072 / Q - 1); }
    else if (kind(s) === 2) assert.ok(ev.length === 0 && r.state.state[s] === 1 && r.timers.waited[s] === 0);
    else if (kind(s) === 3) { assert.deepStrictEqual(ev, [['progress', NAK], ['progress', ACK], ['progress', ACK], ['done', ACK]]); assert.strictEqual(r.state.packetsSent[s], 3); }
    else { assert.deepStrictEqual(ev, [['progress', NAK], ['progress', EOT], ['aborted', -1]]); assert.ok(r.when[s][2] > r.when[s][1] + 3072 / Q - 2); }
  }
  console.log('js xmodem timer gpu tests ok');
}

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
