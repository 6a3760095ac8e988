// Golden-vector harness for the resident XModem sender (TEST INFRASTRUCTURE, build container only).
//
// Drives the REAL XModemTransport.sendData() (type-stripped into a temp dir by oracle/refrun/strip_ts.py, never committed) under
// Node 12 through a scripted data channel.  A scenario is a file, {maxPayloadSize, maxRetries} and a list of demodulate() replies;
// a reply is a byte chunk or 'T' -- nothing arrives and the wait's own timeout signal ends it.  Recorded: every modulate() call's
// bytes and how many replies had been handed out before it, the outcome (resolved, or the error's text), getStatistics() and the
// transport's send words afterwards.  Node 12 lacks AbortController and AbortSignal.timeout / .any: minimal stand-ins with the
// standard semantics, as oracle/refrun/golden_harness_next.js has them.
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
  constructor(replies) { this.replies = replies; this.taken = 0; this.sent = []; this.ranOut = false; }
  async modulate(data) { this.sent.push({ bytes: Uint8Array.from(data), after: this.taken }); }
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
const rand = rng32(0x7E5D);
function file(n) { const p = new Uint8Array(n); for (let i = 0; i < n; i++) p[i] = Math.floor(rand() * 256); return p; }

const ACK = [0x06], NAK = [0x15], EOT = [0x04], T = 'T';
function rep(x, n) { const out = []; for (let i = 0; i < n; i++) out.push(x); return out; }
// name, file length, maxPayloadSize, maxRetries, replies
const SCENARIOS = [
  ['one_fragment', 10, 128, 10, [NAK, ACK, ACK]],
  ['two_fragments', 200, 128, 10, [NAK, ACK, ACK, ACK]],
  ['five_fragments', 75, 16, 10, [NAK].concat(rep(ACK, 6))],
  ['empty_file', 0, 128, 10, [NAK, ACK, ACK]],
  ['exact_multiple', 64, 16, 10, [NAK].concat(rep(ACK, 5))],
  ['sequence_wraps', 300, 1, 10, [NAK].concat(rep(ACK, 301))],
  ['longest_payload', 255, 255, 10, [NAK, ACK, ACK]],
  ['nak_answered_once', 40, 16, 10, [NAK, ACK, NAK, ACK, ACK, ACK]],
  ['naks_up_to_max_retries', 20, 16, 3, [NAK, ACK, NAK, NAK, NAK, ACK, ACK]],
  ['naks_beyond_max_retries', 20, 16, 3, [NAK, ACK, NAK, NAK, NAK, NAK, ACK, ACK]],
  ['max_retries_zero', 5, 16, 0, [NAK, NAK, ACK]],
  ['retries_are_per_fragment', 48, 16, 2, [NAK, NAK, NAK, ACK, NAK, NAK, ACK, NAK, NAK, ACK, ACK]],
  ['control_behind_noise', 20, 16, 10, [[0x00, 0x41, 0x01, 0x15], [0x7F, 0x06], [0x55, 0xAA, 0x06, 0x33], [0x99, 0x06]]],
  ['second_control_is_lost', 40, 16, 10, [[0x15, 0x06], [0x06, 0x06], ACK, ACK, ACK]],
  ['ack_then_nak_in_one_reply', 20, 16, 10, [NAK, [0x06, 0x15], ACK, ACK]],
  ['nak_then_ack_in_one_reply', 20, 16, 10, [NAK, [0x15, 0x06], ACK, ACK, ACK]],
  ['eot_while_waiting_for_ack', 20, 16, 10, [NAK, EOT, [0x04, 0x06], ACK, ACK, ACK]],
  ['ack_and_eot_before_first_nak', 10, 16, 10, [ACK, EOT, [0x06, 0x15], NAK, ACK, ACK]],
  ['own_eot_echo_before_final_ack', 10, 16, 10, [NAK, ACK, EOT, [0x04, 0x15, 0x06]]],
  ['nak_in_final_wait_is_ignored', 10, 16, 10, [NAK, ACK, NAK, [0x15, 0x04], ACK]],
  ['final_ack_behind_noise', 10, 16, 10, [NAK, ACK, [0x01, 0x02, 0xFF, 0x06, 0x15]]],
  ['empty_reply', 20, 16, 10, [[], NAK, [], ACK, [], [], ACK, [], ACK]],
  ['only_noise_replies', 10, 16, 10, [[0x41, 0x42], NAK, [0x01, 0x01, 0x00], ACK, [0x15 ^ 0xFF], ACK]],
  ['timeout_in_first_wait', 10, 16, 10, [T]],
  ['timeout_in_first_wait_after_skips', 10, 16, 10, [ACK, [], T]],
  ['timeout_in_ack_wait', 40, 16, 10, [NAK, ACK, T]],
  ['timeout_in_ack_wait_after_nak', 40, 16, 10, [NAK, NAK, T]],
  ['timeout_in_final_wait', 10, 16, 10, [NAK, ACK, T]],
  ['timeout_in_final_wait_after_echo', 10, 16, 10, [NAK, ACK, EOT, T]],
];

async function run(name, fileLen, maxPayloadSize, maxRetries, replies) {
  const data = file(fileLen);
  const ch = new ScriptChannel(replies);
  const t = new R.XModemTransport(ch);
  t.configure({ timeoutMs: 5, maxRetries, maxPayloadSize });
  let outcome = null;
  try { await t.sendData(data); } catch (e) { outcome = e.message; }
  if (ch.ranOut) throw new Error(name + ': the script ran out of replies');
  const st = t.getStatistics();
  return { name, data, maxPayloadSize, maxRetries, replies, sent: ch.sent, outcome, taken: ch.taken,
    stats: { packetsSent: st.packetsSent, packetsRetransmitted: st.packetsRetransmitted, packetsReceived: st.packetsReceived, packetsDropped: st.packetsDropped,
      bytesTransferred: st.bytesTransferred },
    after: { state: t.getCurrentState(), sequence: t.send.sequence, fragmentIndex: t.send.fragmentIndex, fragments: t.send.fragments.length, retries: t.send.retries } };
}

async function busyText() {   // sendData on a transport that is inside sendData: ensureIdle's message, per state
  const out = {};
  for (const [key, replies] of [['SENDING_WAIT_NAK', [T]], ['SENDING_WAIT_ACK', [NAK, T]], ['SENDING_WAIT_FINAL_ACK', [NAK, ACK, T]]]) {
    const ch = new ScriptChannel(replies);
    const t = new R.XModemTransport(ch);
    t.configure({ timeoutMs: 20, maxRetries: 10, maxPayloadSize: 16 });
    const first = t.sendData(Uint8Array.from([1, 2, 3])).catch(() => {});
    await new Promise(r => setTimeout(r, 2));
    try { await t.sendData(Uint8Array.from([4])); out[key] = null; } catch (e) { out[key] = e.message; }
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
  const results = [];
  let busy;
  try {
    for (const sc of SCENARIOS) results.push(await run(...sc));
    busy = await busyText();
  } finally { console.log = log; console.warn = warn; }
  const files = [], replies = [], kinds = [], sent = [], after = [], cases = [];
  for (const r of results) {
    cases.push({ name: r.name, file: files.length, maxPayloadSize: r.maxPayloadSize, maxRetries: r.maxRetries, reply_first: replies.length, reply_count: r.replies.length,
      replies_taken: r.taken, sent_first: sent.length, sent_count: r.sent.length, outcome: r.outcome, stats: r.stats, after: r.after });
    files.push(r.data);
    for (const x of r.replies) { kinds.push(x === 'T' ? 1 : 0); replies.push(x === 'T' ? [] : x); }
    for (const m of r.sent) { sent.push(m.bytes); after.push(m.after); }
  }
  saveRagged('file', files); saveRagged('reply', replies); saveRagged('sent', sent);
  fs.writeFileSync(path.join(OUT, 'reply.timeout.u1.bin'), Buffer.from(Uint8Array.from(kinds)));
  const aft = Int32Array.from(after);
  fs.writeFileSync(path.join(OUT, 'sent.after.i4.bin'), Buffer.from(aft.buffer, aft.byteOffset, aft.byteLength));
  const manifest = { generator: 'tools/xmodem_tx_golden/harness.js', node: process.version, busy, cases,
    arrays: ['file.data.u1', 'file.off.i4', 'reply.data.u1', 'reply.off.i4', 'reply.timeout.u1', 'sent.data.u1', 'sent.off.i4', 'sent.after.i4'] };
  fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest));
}
main().catch(e => { console.error(e); process.exit(1); });
