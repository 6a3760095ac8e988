// Golden-vector harness for the resident XModem file receiver (TEST INFRASTRUCTURE, build container only).
//
// Drives the REAL XModemTransport.receiveData() (type-stripped into a temp dir by oracle/refrun/strip_ts.py, never committed) under
// Node through a scripted data channel.  A scenario is {maxRetries}, a list of demodulate() replies -- a reply is a byte chunk or
// 'T': nothing arrives and the wait's own timeout signal ends it -- and optionally abortAtSend: the external signal is aborted
// inside that modulate() call, so that the loop's checkAbort sees it next.  modulate() resolves at once.  Recorded: every
// modulate() call's bytes and how many replies had been handed out before it, the outcome (the returned bytes, or the error's
// text), getStatistics(), expectedSequence, send.retries and the state afterwards, and ensureIdle's message per state.  Node
// versions without AbortController / AbortSignal.timeout / .any get minimal stand-ins with the standard semantics, as
// tools/xmodem_tx_golden/harness.js has them.
//
// usage: node harness.js <ref_bundle.js> <out_dir>
'use strict';
const fs = require('fs');
const path = require('path');
const R = require(path.resolve(process.argv[2]));
const OUT = process.argv[3];
fs.mkdirSync(OUT, { recursive: true });

class MiniSignal {
  constructor() { this.aborted = false; this.reason = undefined; this._l = []; }
  addEventListener(t, f) { if (t === 'abort') this._l.push(f); }
  removeEventListener(t, f) { this._l = this._l.filter(x => x !== f); }
  _fire(reason) { if (this.aborted) return; this.aborted = true; this.reason = reason; this._l.slice().forEach(f => f()); }
}
global.AbortController = class { constructor() { this.signal = new MiniSignal(); } abort(r) { this.signal._fire(r || new Error('This operation was aborted')); } };
global.AbortSignal = {
  timeout(ms) { const s = new MiniSignal(); setTimeout(() => s._fire(new Error('The operation was aborted due to timeout')), ms); return s; },
  any(list) { const s = new MiniSignal(); for (const x of list) { if (x.aborted) { s._fire(x.reason); break; } x.addEventListener('abort', () => s._fire(x.reason)); } return s; },
};

class ScriptChannel {   // IDataChannel: modulate records what the transport sends, demodulate hands out the script one reply per call
  constructor(replies, opts) { this.replies = replies; this.taken = 0; this.sent = []; this.ranOut = false; this.opts = opts || {}; }
  async modulate(data) {
    this.sent.push({ bytes: Uint8Array.from(data), after: this.taken });
    if (this.opts.abortAtSend === this.sent.length) this.opts.controller.abort();
    if (this.opts.sendDelay && this.opts.sendDelay[this.sent.length - 1]) await new Promise(r => setTimeout(r, this.opts.sendDelay[this.sent.length - 1]));
  }
  async demodulate(options) {
    let reply = 'T';
    if (this.taken < this.replies.length) reply = this.replies[this.taken++]; else this.ranOut = true;
    if (reply !== 'T') return Uint8Array.from(reply);
    return new Promise((resolve, reject) => {   // nothing arrives: only the caller's timeout signal ends the wait
      const sig = options && options.signal;
      if (!sig) return;
      if (sig.aborted) { reject(new Error('Demodulation aborted')); return; }
      sig.addEventListener('abort', () => reject(new Error('Demodulation aborted')));
    });
  }
  reset() {}
}

function rng32(seed) {
  let a = seed >>> 0;
  return function () {
    a = (a + 0x6D2B79F5) >>> 0;
    let t = a;
    t = Math.imul(t ^ (t >>> 15), t | 1);
    t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
}
const rand = rng32(0x4EC5);
function bytes(n) { const p = []; for (let i = 0; i < n; i++) p.push(Math.floor(rand() * 256)); return p; }
function crc16(data) {   // CRC-16-CCITT, 0x1021, initial 0xFFFF: the scenario's input bytes, not the code under test
  let c = 0xFFFF;
  for (const b of data) { c ^= b << 8; for (let k = 0; k < 8; k++) c = (c & 0x8000) ? ((c << 1) ^ 0x1021) & 0xFFFF : (c << 1) & 0xFFFF; }
  return c;
}
function pkt(seq, payload, o) {
  o = o || {};
  const c = crc16(payload) ^ (o.crcXor || 0);
  return [0x01, seq, o.inv === undefined ? 255 - seq : o.inv, payload.length].concat(payload, [c >> 8, c & 0xFF]);
}
const EOT = [0x04], T = 'T';
function rep(x, n) { const out = []; for (let i = 0; i < n; i++) out.push(x); return out; }
function cat() { return [].concat.apply([], arguments); }

const P1 = bytes(10), P2 = bytes(128), P3 = bytes(1), P4 = bytes(33), P5 = bytes(255);
const five = [1, 2, 3, 4, 5].map(s => pkt(s, bytes(16)));
const wrap = []; for (let i = 0; i < 257; i++) wrap.push(pkt(i % 255 + 1, [i & 0xFF]));
const p1 = pkt(1, P1), p2 = pkt(2, P2), p3 = pkt(3, P3);
const badCrc = pkt(1, P1, { crcXor: 0x0100 }), badInv = pkt(1, P1, { inv: 0x00 }), unexpected = pkt(7, P4);
// name, maxRetries, replies, options
const SCENARIOS = [
  ['one_packet', 10, [p1, EOT]],
  ['two_packets', 10, [p1, p2, EOT]],
  ['five_packets', 10, five.concat([EOT])],
  ['empty_file', 10, [pkt(1, []), EOT]],
  ['eot_with_no_packet', 10, [EOT]],
  ['two_packets_and_eot_in_one_reply', 10, [cat(p1, p2, EOT)]],
  ['longest_payload', 10, [pkt(1, P5), EOT]],
  ['packet_split_across_three_replies', 10, [p1.slice(0, 2), p1.slice(2, 9), p1.slice(9), EOT]],
  ['split_at_every_boundary', 10, [[0x01], [1], [254, 10], P1.slice(0, 10), p1.slice(14, 15), p1.slice(15), EOT]],
  ['noise_before_soh_and_between_packets', 10, [cat([0x00, 0x41, 0xFF], p1), cat([0x06, 0x15], p2, [0x7F]), cat([0x55], EOT)]],
  ['only_noise_replies', 10, [[0x41, 0x42], p1, [0x00], [], EOT]],
  ['duplicate', 10, [p1, p1, p2, EOT]],
  ['duplicate_does_not_reset_retries', 2, [p1, badCrc.map((b, i) => i === 1 ? 2 : i === 2 ? 253 : b), p1, pkt(2, P2, { crcXor: 1 }), pkt(2, P2, { crcXor: 2 }), p2, EOT]],
  ['invalid_crc_then_good', 10, [badCrc, p1, EOT]],
  ['invalid_sequence_then_good', 10, [badInv, p1, EOT]],
  ['unexpected_sequence_then_good', 10, [unexpected, p1, EOT]],
  ['error_clears_what_arrived_with_it', 10, [cat(badCrc, p1), p1, EOT]],
  ['errors_up_to_max_retries', 3, [badCrc, badInv, unexpected, p1, EOT]],
  ['errors_beyond_max_retries', 3, [badCrc, badInv, unexpected, badCrc, p1, EOT]],
  ['max_retries_zero', 0, [badCrc, p1]],
  ['retries_reset_by_an_accepted_packet', 2, [badCrc, badCrc, p1, pkt(2, P2, { crcXor: 5 }), pkt(2, P2, { inv: 9 }), p2, EOT]],
  ['sequence_wraps', 10, wrap.concat([EOT])],
  ['duplicate_of_255_when_expecting_1', 10, wrap.slice(0, 255).concat([wrap[254], wrap[255], EOT])],
  ['timeout_in_first_byte_wait', 10, [T, p1, EOT]],
  ['timeout_in_header_wait', 10, [p1.slice(0, 2), T, p1, EOT]],
  ['timeout_in_payload_wait', 10, [p1.slice(0, 9), T, p1, EOT]],
  ['timeouts_beyond_max_retries', 2, [T, T, T]],
  ['timeout_then_error_beyond_max_retries', 1, [T, badCrc]],
  ['bytes_behind_the_eot', 10, [p1, cat(EOT, [0x01, 0x02, 0x03])]],
  ['external_abort', 10, [p1, p2], { abortAtSend: 3 }],
  ['external_abort_before_any_packet', 10, [], { abortAtSend: 1 }],
];

async function run(name, maxRetries, replies, opts) {
  opts = Object.assign({}, opts || {});
  const controller = new AbortController();
  opts.controller = controller;
  const ch = new ScriptChannel(replies, opts);
  const t = new R.XModemTransport(ch);
  t.configure({ timeoutMs: 5, maxRetries, maxPayloadSize: 128 });
  let outcome = null, result = null;
  try { result = await t.receiveData({ signal: controller.signal }); } catch (e) { outcome = e.message; }
  if (ch.ranOut && !(outcome && /max retries/.test(outcome))) throw new Error(name + ': the script ran out of replies');
  const st = t.getStatistics();
  return { name, maxRetries, replies, sent: ch.sent, outcome, result, taken: ch.taken, abort: opts.abortAtSend ? 1 : 0,
    statistics: { packetsSent: st.packetsSent, packetsRetransmitted: st.packetsRetransmitted, packetsReceived: st.packetsReceived, packetsDropped: st.packetsDropped,
      bytesTransferred: st.bytesTransferred },
    expectedSequence: t.receive.expectedSequence, retries: t.send.retries, state: t.getCurrentState() };
}

async function busyText() {   // receiveData on a transport that is inside receiveData: ensureIdle's message, per state
  const out = {};
  for (const [key, replies, sendDelay] of [['RECEIVING_SEND_NAK', [T], [20]], ['RECEIVING_WAIT_BLOCK', [T], []], ['RECEIVING_SEND_ACK', [p1, T], [0, 20]]]) {
    const ch = new ScriptChannel(replies, { sendDelay });
    const t = new R.XModemTransport(ch);
    t.configure({ timeoutMs: 30, maxRetries: 0, maxPayloadSize: 128 });
    const first = t.receiveData().catch(() => {});
    await new Promise(r => setTimeout(r, 4));
    try { await t.receiveData(); out[key] = null; } catch (e) { out[key] = e.message; }
    await first;
  }
  return out;
}

function saveRagged(name, list) {
  const off = new Int32Array(list.length + 1);
  let n = 0;
  list.forEach((a, i) => { off[i] = n; n += a.length; });
  off[list.length] = n;
  const data = new Uint8Array(n);
  list.forEach((a, i) => data.set(a, off[i]));
  fs.writeFileSync(path.join(OUT, name + '.data.u1.bin'), Buffer.from(data.buffer, data.byteOffset, data.byteLength));
  fs.writeFileSync(path.join(OUT, name + '.off.i4.bin'), Buffer.from(off.buffer, off.byteOffset, off.byteLength));
}

async function main() {
  const log = console.log, warn = console.warn;
  console.log = () => {}; console.warn = () => {};
  const runs = [];
  let busy;
  try {
    for (const sc of SCENARIOS) runs.push(await run(...sc));
    busy = await busyText();
  } finally { console.log = log; console.warn = warn; }
  const results = [], replies = [], kinds = [], sent = [], after = [], cases = [];
  for (const r of runs) {
    cases.push({ name: r.name, maxRetries: r.maxRetries, reply_first: replies.length, reply_count: r.taken, sent_first: sent.length, sent_count: r.sent.length,
      outcome: r.outcome, result: r.result ? results.length : -1, abort: r.abort, statistics: r.statistics, expectedSequence: r.expectedSequence, retries: r.retries,
      state: r.state });
    if (r.result) results.push(r.result);
    for (const x of r.replies.slice(0, r.taken)) { kinds.push(x === 'T' ? 1 : 0); replies.push(x === 'T' ? [] : x); }
    for (const m of r.sent) { sent.push(m.bytes); after.push(m.after); }
  }
  saveRagged('result', results); saveRagged('reply', replies); saveRagged('sent', sent);
  fs.writeFileSync(path.join(OUT, 'reply.timeout.u1.bin'), Buffer.from(Uint8Array.from(kinds)));
  const aft = Int32Array.from(after);
  fs.writeFileSync(path.join(OUT, 'sent.after.i4.bin'), Buffer.from(aft.buffer, aft.byteOffset, aft.byteLength));
  const manifest = { generator: 'tools/xmodem_recv_golden/harness.js', node: process.version, busy, cases,
    arrays: ['result.data.u1', 'result.off.i4', 'reply.data.u1', 'reply.off.i4', 'reply.timeout.u1', 'sent.data.u1', 'sent.off.i4', 'sent.after.i4'] };
  fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest));
}
main().catch(e => { console.error(e); process.exit(1); });
