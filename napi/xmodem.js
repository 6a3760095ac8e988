'use strict';
// CRC16 / XModemPacket / ControlType with the reference's surface (src/utils/crc16.ts, src/transports/xmodem/packet.ts,
// types.ts), plus the batch forms and scanBursts -- the receive checks of XModemTransport (xmodem.ts:233-320) applied
// to recorded bursts -- and XModemReceiverBatch, the same grammar resident on the device over the RX rings of an
// FSKProcessorBatch.  Everything that COMPUTES does so in libfskhip.so through the N-API addon (no JavaScript CRC here); the one
// method that only lays bytes out is XModemPacket.serialize(packet): packet.ts:44-54 writes the fields of the packet OBJECT as
// they are -- checksum included, whatever it holds (the reference's tests serialise packets with a wrong one) -- so it cannot go
// through serializeBatch, which computes the CRC.
const path = require('path');
const addon = require(path.join(__dirname, 'fsk_addon.node'));

const ControlType = Object.freeze({ SOH: 0x01, ACK: 0x06, NAK: 0x15, EOT: 0x04 });      // types.ts:29-34
const PacketConstants = Object.freeze({ SOH: 0x01, HEADER_SIZE: 4, CRC_SIZE: 2, MIN_PACKET_SIZE: 6, MAX_PACKET_SIZE: 261,
  MAX_PAYLOAD_SIZE: 255, MAX_SEQUENCE: 255, MIN_DATA_SEQUENCE: 1 });                       // types.ts:62-75
const XM_STATUS = ['need_more', 'eot', 'truncated', 'invalid_sequence', 'invalid_crc', 'unexpected_sequence'];
const XM_ERRORS = { 3: 'Invalid sequence number', 4: 'Invalid CRC', 5: 'Unexpected sequence number' };  // xmodem.ts:273,290,318

function packRows(rows) {
  let mx = 0;
  for (const r of rows) mx = Math.max(mx, r.length);
  const pitch = Math.max(4, (mx + 3) & ~3);
  const slab = new Uint8Array(pitch * rows.length);
  const lens = new Uint32Array(rows.length);
  rows.forEach((r, i) => { slab.set(r, i * pitch); lens[i] = r.length; });
  return { slab, pitch, lens };
}

function crc16Batch(rows, device = 0) {
  if (!rows.length) return new Uint16Array(0);
  const p = packRows(rows);
  return addon.crc16(p.slab, p.pitch, p.lens, device);
}

class CRC16 {                                   // crc16.ts:11-50
  static calculate(data, device = 0) { return crc16Batch([data], device)[0]; }
  static verify(data, expectedCrc, device = 0) { return CRC16.calculate(data, device) === expectedCrc; }
}

function serializeBatch(seqs, payloads, device = 0) {
  seqs.forEach((sequence, i) => {               // createData's throws (packet.ts:22-27)
    if (sequence < 1 || sequence > 255) throw new Error(`Invalid sequence: ${sequence}. Must be 1-255.`);
    if (payloads[i].length > 255) throw new Error(`Payload too large: ${payloads[i].length}. Max 255 bytes.`);
  });
  if (!seqs.length) return [];
  const p = packRows(payloads);
  const r = addon.xmodemSerialize(p.slab, p.pitch, p.lens, Uint32Array.from(seqs), device);
  return payloads.map((_, i) => r.out.slice(i * r.outPitch, i * r.outPitch + r.lens[i]));
}

class XModemPacket {                            // packet.ts:17-66
  static createData(sequence, payload, device = 0) {
    const wire = serializeBatch([sequence], [payload], device)[0];
    return { soh: wire[0], sequence: wire[1], invSequence: wire[2], length: wire[3], payload: new Uint8Array(payload),
      checksum: (wire[wire.length - 2] << 8) | wire[wire.length - 1] };
  }
  static serialize(packet) {
    const result = new Uint8Array(4 + packet.payload.length + 2);
    result[0] = packet.soh; result[1] = packet.sequence; result[2] = packet.invSequence; result[3] = packet.length;
    result.set(packet.payload, 4);
    result[4 + packet.payload.length] = (packet.checksum >> 8) & 0xFF;
    result[4 + packet.payload.length + 1] = packet.checksum & 0xFF;
    return result;
  }
  static verify(packet, device = 0) { return CRC16.calculate(packet.payload, device) === packet.checksum; }
  static serializeControl(controlType) { return new Uint8Array([controlType]); }
}

// bursts: array of Uint8Array (what the demodulator returned per stream); expected: starting expectedSequence per stream
const resultOf = (q) => ({ status: q[0], statusName: XM_STATUS[q[0]], error: XM_ERRORS[q[0]] || null, expectedAfter: q[1], packets: q[2], dropped: q[3],
  consumed: q[4], errSeq: q[6], errLen: q[7], crcRx: q[8], crcCalc: q[9] });

function scanBursts(bursts, expected, device = 0) {
  if (!bursts.length) return [];
  const p = packRows(bursts);
  const exp = Uint32Array.from(bursts.map((_, i) => (Array.isArray(expected) || ArrayBuffer.isView(expected)) ? expected[i] : expected));
  const r = addon.xmodemScan(p.slab, p.pitch, p.lens, exp, device);
  return bursts.map((_, i) => {
    const q = r.results.subarray(i * 10, i * 10 + 10);
    return Object.assign(resultOf(q), { data: r.data.slice(i * r.dataPitch, i * r.dataPitch + q[5]) });
  });
}

// The receive side of XModemTransport for every stream of an FSKProcessorBatch (fsk-processor.js), resident on the device
// (fskhip_xmodem_rx_*).  poll() walks the RX rings in place and takes whole packets out of them; a packet that has only partly arrived
// waits in its ring, an error clears the ring, bytes behind an EOT stay.  expectedSequence and the running packetsReceived /
// packetsDropped live with this object.  Sending ACK / NAK, retries and timeouts are the caller's.  Close it before its processor.
function stateArray(name, a, n) {
  if (a === undefined || a === null) return null;
  if (!Array.isArray(a) && !ArrayBuffer.isView(a)) throw new TypeError('setState: ' + name + ' must be an array of nStreams integers');
  if (a.length !== n) throw new RangeError('setState: ' + name + ' must have one entry per stream (' + n + ')');
  for (const v of a) if (!Number.isInteger(v) || v < 0 || v > 0xffffffff) throw new RangeError('setState: ' + name + ' must hold integers in [0, 2^32)');
  return Uint32Array.from(a);
}
class XModemReceiverBatch {
  constructor(processor) {
    if (processor === null || typeof processor !== 'object' || !Number.isInteger(processor.nStreams)) throw new TypeError('XModemReceiverBatch: processor must be an FSKProcessorBatch');
    this.processor = processor;
    this.nStreams = processor.nStreams;
    this.handle = addon.xmodemRxCreate(processor.handle);
  }
  close() { if (this.handle) { addon.xmodemRxDestroy(this.handle); this.handle = null; } }
  // {streams, results, offsets, data}: the streams with an event in ascending order, one result each (scanBursts' fields, `data`
  // the accepted payload of that stream), and the same payloads in CSR form: data.subarray(offsets[i], offsets[i + 1])
  poll(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('poll: options must be an object {mask}');
    const { mask } = options;
    let m = null;
    if (mask !== undefined && mask !== null) {
      if (!Array.isArray(mask) && !ArrayBuffer.isView(mask)) throw new TypeError('poll: mask must be an array of nStreams booleans');
      if (mask.length !== this.nStreams) throw new RangeError('poll: mask must have one entry per stream (' + this.nStreams + ')');
      m = Uint8Array.from(mask, (b) => (b ? 1 : 0));
    }
    const r = addon.xmodemRxPoll(this.handle, m);
    const results = Array.from(r.streams, (_, i) =>
      Object.assign(resultOf(r.results.subarray(i * 10, i * 10 + 10)), { data: r.data.slice(r.offsets[i], r.offsets[i + 1]) }));
    return { streams: r.streams, results, offsets: r.offsets, data: r.data };
  }
  // initializeReceive() (xmodem.ts:221-225): expectedSequence = 1 for one stream, or all (-1)
  reset(stream = -1) {
    if (!Number.isInteger(stream)) throw new TypeError('reset: stream must be an integer (-1: all)');
    addon.xmodemRxReset(this.handle, stream);
  }
  state() { return addon.xmodemRxState(this.handle); }                 // {expected, packets, dropped}: Uint32Array per stream
  setState(state) {                                                     // what state() returned, or any part of it (expected: 1..255)
    if (state === null || typeof state !== 'object') throw new TypeError('setState: state must be an object {expected, packets, dropped}');
    const n = this.nStreams;
    addon.xmodemRxSetState(this.handle, stateArray('expected', state.expected, n), stateArray('packets', state.packets, n), stateArray('dropped', state.dropped, n));
  }
}

// The send side of XModemTransport for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_tx_*): send() hands
// each stream a file, poll() takes what each waiting stream's RX ring holds as ONE demodulate() reply and, where the control byte a wait
// is waiting for has arrived, builds the next packet (or the EOT) on the device and starts its modulation.  What a poll finds depends
// on when it happens, as in the reference.  The timers are the caller's: poll({abort}) ends the waits that have lasted too long.
const TX_STATES = ['IDLE', 'SENDING_WAIT_NAK', 'SENDING_WAIT_ACK', 'SENDING_WAIT_FINAL_ACK'];
const TX_STATUS = ['progress', 'done', 'max_retries', 'aborted'];
const TX_ERRORS = [null, null, 'Timeout - max retries exceeded', 'Operation aborted'];
const TX_WORDS = ['state', 'sequence', 'fragmentIndex', 'retries', 'packetsSent', 'retransmitted'];
function boolArray(who, name, a, n) {
  if (a === undefined || a === null) return null;
  if (!Array.isArray(a) && !ArrayBuffer.isView(a)) throw new TypeError(who + ': ' + name + ' must be an array of nStreams booleans');
  if (a.length !== n) throw new RangeError(who + ': ' + name + ' must have one entry per stream (' + n + ')');
  return Uint8Array.from(a, (b) => (b ? 1 : 0));
}
// what a sender's poll returns, from the addon's {streams, events: Int32Array[8 * n]}
function txPolled(r) {
  const events = Array.from(r.streams, (_, i) => {
    const q = r.events.subarray(i * 8, i * 8 + 8);
    return { status: q[0], statusName: TX_STATUS[q[0]], error: TX_ERRORS[q[0]], stateAfter: q[1], stateName: TX_STATES[q[1]], control: q[2], sentLen: q[3],
      sequence: q[4], fragmentIndex: q[5], nFragments: q[6], retries: q[7] };
  });
  return { streams: r.streams, events };
}
class XModemSenderBatch {
  constructor(processor, options = {}) {
    if (processor === null || typeof processor !== 'object' || !Number.isInteger(processor.nStreams)) throw new TypeError('XModemSenderBatch: processor must be an FSKProcessorBatch');
    if (options === null || typeof options !== 'object') throw new TypeError('XModemSenderBatch: options must be an object {maxPayloadSize, maxRetries}');
    const { maxPayloadSize = 128, maxRetries = 10 } = options;
    if (!Number.isInteger(maxPayloadSize) || maxPayloadSize < 1 || maxPayloadSize > 255) throw new RangeError('XModemSenderBatch: maxPayloadSize must be an integer in 1..255');
    if (!Number.isInteger(maxRetries) || maxRetries < 0 || maxRetries > 0xffffffff) throw new RangeError('XModemSenderBatch: maxRetries must be an integer in [0, 2^32)');
    this.processor = processor;
    this.nStreams = processor.nStreams;
    this.maxPayloadSize = maxPayloadSize;
    this.maxRetries = maxRetries;
    this.handle = addon.xmodemTxCreate(processor.handle, maxPayloadSize, maxRetries);
  }
  close() { if (this.handle) { addon.xmodemTxDestroy(this.handle); this.handle = null; } }
  // sendData(files[s]) for every stream, or those of options.mask (the other entries are ignored).  Nothing is transmitted yet; a stream
  // that is still sending throws the reference's 'Transport busy' text and nothing is started.
  send(files, options = {}) {
    if (!Array.isArray(files)) throw new TypeError('send: files must be an array of nStreams byte arrays');
    if (files.length !== this.nStreams) throw new RangeError('send: files must have one entry per stream (' + this.nStreams + ')');
    if (options === null || typeof options !== 'object') throw new TypeError('send: options must be an object {mask}');
    const m = boolArray('send', 'mask', options.mask, this.nStreams);
    const rows = files.map((f, s) => {
      if (m && !m[s]) return new Uint8Array(0);
      if (!Array.isArray(f) && !ArrayBuffer.isView(f)) throw new TypeError('send: files[' + s + '] must be a byte array');
      return Uint8Array.from(f);
    });
    const offsets = new Uint32Array(this.nStreams + 1);
    let total = 0;
    rows.forEach((r, s) => { offsets[s] = total; total += r.length; });
    if (total > 0xffffffff) throw new RangeError('send: the files together exceed 2^32 - 1 bytes');
    offsets[this.nStreams] = total;
    const data = new Uint8Array(total);
    rows.forEach((r, s) => data.set(r, offsets[s]));
    addon.xmodemTxSend(this.handle, m, offsets, data);
  }
  // {streams, events}: the streams where something happened in ascending order, and one event each
  poll(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('poll: options must be an object {mask, abort}');
    const m = boolArray('poll', 'mask', options.mask, this.nStreams), a = boolArray('poll', 'abort', options.abort, this.nStreams);
    return txPolled(addon.xmodemTxPoll(this.handle, m, a));
  }
  // reset() (xmodem.ts:370-383) for one stream, or all (-1): IDLE, sequence 1, the file dropped, the counters 0
  reset(stream = -1) {
    if (!Number.isInteger(stream)) throw new TypeError('reset: stream must be an integer (-1: all)');
    addon.xmodemTxReset(this.handle, stream);
  }
  state() { return addon.xmodemTxState(this.handle); }   // {state, sequence, fragmentIndex, retries, packetsSent, retransmitted}: Uint32Array per stream
  setState(state) {                                       // what state() returned, or any part of it, after send() on this object
    if (state === null || typeof state !== 'object') throw new TypeError('setState: state must be an object {' + TX_WORDS.join(', ') + '}');
    addon.xmodemTxSetState(this.handle, ...TX_WORDS.map((k) => stateArray(k, state[k], this.nStreams)));
  }
}

// receiveData() of XModemTransport for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_recv_*): start() sends
// the initial NAK, poll() walks each waiting stream's RX ring up to the first step of the receive grammar that owes a reply, appends an
// accepted payload to the stream's file on the device, counts retries and starts the ACK or NAK on the processor.  Only events come back;
// files() reads the assembled files once, at the end.  The timers are the caller's: poll({timeout}) names the streams whose wait's timer
// has fired, poll({abort}) the streams to abort.
const RECV_STATES = ['IDLE', 'RECEIVING_SEND_NAK', 'RECEIVING_WAIT_BLOCK', 'RECEIVING_SEND_ACK'];
const RECV_STATUS = ['progress', 'done', 'max_retries', 'aborted', 'file_full'];
const RECV_ERRORS = [null, null, 'Receive failed after max retries', 'Operation aborted', 'File store full'];
const RECV_WORDS = ['state', 'expected', 'retries', 'fileLen', 'packetsReceived', 'dropped', 'packetsSent'];
// what a file receiver's poll returns, from the addon's {streams, events: Int32Array[12 * n]}
function recvPolled(r) {
  const events = Array.from(r.streams, (_, i) => {
    const q = r.events.subarray(i * 12, i * 12 + 12);
    return { status: q[0], statusName: RECV_STATUS[q[0]], error: RECV_ERRORS[q[0]], stateAfter: q[1], stateName: RECV_STATES[q[1]], control: q[2], step: q[3],
      stepName: XM_STATUS[q[3]], seq: q[4], len: q[5], acceptedLen: q[6], fileLen: q[7], expected: q[8], retries: q[9], crcRx: q[10], crcCalc: q[11] };
  });
  return { streams: r.streams, events };
}
class XModemFileReceiverBatch {
  constructor(processor, options = {}) {
    if (processor === null || typeof processor !== 'object' || !Number.isInteger(processor.nStreams)) throw new TypeError('XModemFileReceiverBatch: processor must be an FSKProcessorBatch');
    if (options === null || typeof options !== 'object') throw new TypeError('XModemFileReceiverBatch: options must be an object {fileCapacity, maxRetries}');
    const { fileCapacity = 65536, maxRetries = 10 } = options;
    if (!Number.isInteger(fileCapacity) || fileCapacity < 0 || fileCapacity > 0xffffffff) throw new RangeError('XModemFileReceiverBatch: fileCapacity must be an integer in [0, 2^32)');
    if (!Number.isInteger(maxRetries) || maxRetries < 0 || maxRetries > 0xffffffff) throw new RangeError('XModemFileReceiverBatch: maxRetries must be an integer in [0, 2^32)');
    this.processor = processor;
    this.nStreams = processor.nStreams;
    this.fileCapacity = fileCapacity;
    this.maxRetries = maxRetries;
    this.handle = addon.xmodemRecvCreate(processor.handle, fileCapacity, maxRetries);
  }
  close() { if (this.handle) { addon.xmodemRecvDestroy(this.handle); this.handle = null; } }
  // receiveData() up to its first wait for every stream, or those of options.mask: the initial NAK is modulated.  A stream that is still
  // receiving, or whose processor is mid-modulation, throws the reference's text and nothing is started.
  start(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('start: options must be an object {mask}');
    addon.xmodemRecvStart(this.handle, boolArray('start', 'mask', options.mask, this.nStreams));
  }
  // {streams, events}: the streams where something happened in ascending order, and one event each
  poll(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('poll: options must be an object {mask, timeout, abort}');
    const n = this.nStreams;
    return recvPolled(addon.xmodemRecvPoll(this.handle, boolArray('poll', 'mask', options.mask, n), boolArray('poll', 'timeout', options.timeout, n), boolArray('poll', 'abort', options.abort, n)));
  }
  _sel(who, streams) {
    if (streams === undefined || streams === null) return Uint32Array.from({ length: this.nStreams }, (_, i) => i);
    if (!Array.isArray(streams) && !ArrayBuffer.isView(streams)) throw new TypeError(who + ': streams must be an array of stream indices');
    for (const s of streams) if (!Number.isInteger(s) || s < 0 || s >= this.nStreams) throw new RangeError(who + ': streams must hold integers in [0, ' + this.nStreams + ')');
    return Uint32Array.from(streams);
  }
  // the assembled files of `streams` (default: all), one Uint8Array each: packed on the device, one copy
  files(streams) {
    const sel = this._sel('files', streams);
    const r = addon.xmodemRecvFiles(this.handle, sel);
    return Array.from(sel, (_, i) => r.data.slice(r.offsets[i], r.offsets[i + 1]));
  }
  // puts files back (one per stream; those of options.mask, the other entries are ignored): before setState, to carry a receiver across a remap
  setFiles(files, options = {}) {
    if (!Array.isArray(files)) throw new TypeError('setFiles: files must be an array of nStreams byte arrays');
    if (files.length !== this.nStreams) throw new RangeError('setFiles: files must have one entry per stream (' + this.nStreams + ')');
    if (options === null || typeof options !== 'object') throw new TypeError('setFiles: options must be an object {mask}');
    const m = boolArray('setFiles', 'mask', options.mask, this.nStreams);
    const sel = [], rows = [];
    files.forEach((f, s) => {
      if (m && !m[s]) return;
      if (!Array.isArray(f) && !ArrayBuffer.isView(f)) throw new TypeError('setFiles: files[' + s + '] must be a byte array');
      sel.push(s); rows.push(Uint8Array.from(f));
    });
    const offsets = new Uint32Array(sel.length + 1);
    let total = 0;
    rows.forEach((r, i) => { offsets[i] = total; total += r.length; });
    if (total > 0xffffffff) throw new RangeError('setFiles: the files together exceed 2^32 - 1 bytes');
    offsets[sel.length] = total;
    const data = new Uint8Array(total);
    rows.forEach((r, i) => data.set(r, offsets[i]));
    addon.xmodemRecvSetFiles(this.handle, Uint32Array.from(sel), offsets, data);
  }
  // reset() (xmodem.ts:370-383) for one stream, or all (-1): IDLE, expected 1, retries 0, an empty file, the counters 0
  reset(stream = -1) {
    if (!Number.isInteger(stream)) throw new TypeError('reset: stream must be an integer (-1: all)');
    addon.xmodemRecvReset(this.handle, stream);
  }
  state() { return addon.xmodemRecvState(this.handle); }   // {state, expected, retries, fileLen, packetsReceived, dropped, packetsSent}: Uint32Array per stream
  setState(state) {                                         // what state() returned, or any part of it
    if (state === null || typeof state !== 'object') throw new TypeError('setState: state must be an object {' + RECV_WORDS.join(', ') + '}');
    addon.xmodemRecvSetState(this.handle, ...RECV_WORDS.map((k) => stateArray(k, state[k], this.nStreams)));
  }
}

// The `timeoutMs` timers of sendData() / receiveData() for every stream of an XModemFileReceiverBatch or an XModemSenderBatch, resident
// on the device in the engine's sample clock (fskhip_xmodem_timer_*): poll(elapsed) is the handle's own poll between a fire and an arm
// pass, so a receiver's timeout mask and a sender's abort mask are built on the device.  elapsed: the engine samples processed since this
// object's previous poll.  The timers are quantised to the polls (a wait ends at the first poll at or after its deadline): poll once per
// quantum.  The external abort stays the caller's (poll(elapsed, {abort})).  remap / snapshot of the handle do not carry the timers:
// they follow their streams through remap / snapshot / fromSnapshot here, with the same map.  Close it before its handle.
class XModemTimers {
  constructor(handle, options = {}) {
    const recv = handle instanceof XModemFileReceiverBatch;
    if (!recv && !(handle instanceof XModemSenderBatch)) throw new TypeError('XModemTimers: handle must be an XModemFileReceiverBatch or an XModemSenderBatch');
    if (!handle.handle) throw new Error('XModemTimers: the handle has been closed');
    if (options === null || typeof options !== 'object') throw new TypeError('XModemTimers: options must be an object {timeoutSamples} or {timeoutMs, sampleRate}');
    const { timeoutMs, sampleRate = 48000 } = options;
    const timeoutSamples = timeoutMs === undefined ? (options.timeoutSamples === undefined ? 144000 : options.timeoutSamples) : Math.ceil(timeoutMs * sampleRate / 1000);
    if (!Number.isInteger(timeoutSamples) || timeoutSamples < 1 || timeoutSamples > 0xffffffff) throw new RangeError('XModemTimers: the timeout must be an integer number of samples in [1, 2^32)');
    this.over = handle;
    this.recv = recv;
    this.nStreams = handle.nStreams;
    this.timeoutSamples = timeoutSamples;
    this.handle = addon.xmodemTimerCreate(recv, handle.handle, timeoutSamples);
  }
  close() { if (this.handle) { addon.xmodemTimerDestroy(this.handle); this.handle = null; } }
  _live(who) {
    if (!this.handle) throw new Error(who + ': the timers have been closed');
    if (!this.over.handle) throw new Error(who + ": the timers' handle has been closed");
    return this.handle;
  }
  // exactly what the handle's own poll returns
  poll(elapsed, options = {}) {
    if (!Number.isInteger(elapsed) || elapsed < 0 || elapsed > 0xffffffff) throw new RangeError('poll: elapsed must be an integer number of samples in [0, 2^32)');
    if (options === null || typeof options !== 'object') throw new TypeError('poll: options must be an object {mask, abort}');
    const m = boolArray('poll', 'mask', options.mask, this.nStreams), a = boolArray('poll', 'abort', options.abort, this.nStreams);
    const r = addon.xmodemTimerPoll(this._live('poll'), elapsed, m, a);
    return this.recv ? recvPolled(r) : txPolled(r);
  }
  reset(stream = -1) {
    if (!Number.isInteger(stream)) throw new TypeError('reset: stream must be an integer (-1: all)');
    addon.xmodemTimerReset(this._live('reset'), stream);
  }
  state() { return addon.xmodemTimerState(this._live('state')); }   // {waited, mark}: Uint32Array per stream
  setState(state) {                                                  // what state() returned, or either part of it
    if (state === null || typeof state !== 'object') throw new TypeError('setState: state must be an object {waited, mark}');
    addon.xmodemTimerSetState(this._live('setState'), stateArray('waited', state.waited, this.nStreams), stateArray('mark', state.mark, this.nStreams));
  }
  // The timers follow their streams (fskhip_xmodem_timer_remap / _snapshot / _restore): `handle` is the receiver or sender this
  // one's handle was carried into, `map` the map it was carried with.  Stream i of the new object continues the wait of stream
  // map[i] (of record map[i] of an image), -1: a fresh timer.  The timeout is this object's (the image's) unless given.
  remap(handle, map, options = {}) {
    const src = this._live('remap');
    const next = new XModemTimers(handle, { timeoutSamples: options.timeoutSamples === undefined ? this.timeoutSamples : options.timeoutSamples });
    try { addon.xmodemTimerRemap(next.handle, src, Array.from(map)); } catch (e) { next.close(); throw e; }
    return next;
  }
  snapshot(streams) {
    return addon.xmodemTimerSnapshot(this._live('snapshot'), streams === undefined || streams === null ? null : Array.from(streams));
  }
  static fromSnapshot(handle, buf, map, options = {}) {
    const info = xmodemTimerSnapshotInfo(buf);
    const m = map === undefined || map === null ? Array.from({ length: info.nStreams }, (_, i) => i) : Array.from(map);
    const next = new XModemTimers(handle, { timeoutSamples: options.timeoutSamples === undefined ? info.timeoutSamples : options.timeoutSamples });
    try {
      const kind = next.recv ? 'recv' : 'tx';
      if (XM_KINDS[info.kind] !== kind) throw new TypeError(`XModemTimers.fromSnapshot: the snapshot is of kind '${XM_KINDS[info.kind]}', the handle's is '${kind}'`);
      addon.xmodemTimerRestore(next.handle, buf, m);
    } catch (e) { next.close(); throw e; }
    return next;
  }
}
function xmodemTimerSnapshotInfo(buf) { return addon.xmodemTimerSnapshotInfo(buf); }   // {kind (2 tx, 3 recv), nStreams, timeoutSamples}

// remap / snapshot / fromSnapshot of the three resident classes: the handle's state follows its streams with the map the engine and
// the processor were carried with (fskhip_xmodem_{rx,tx,recv}_remap / _snapshot / _restore).  `like(processor)` makes a new object
// with this one's parameters over the destination processor; `made(processor, info, options)` one with an image's.
const XM_KINDS = { 1: 'rx', 2: 'tx', 3: 'recv' };
function xmodemSnapshotInfo(buf) { return addon.xmodemSnapshotInfo(buf); }
function lifecycle(Class, kind, fns, like, made) {
  Class.prototype.remap = function remap(processor, map) {
    const next = like(this, processor);
    try { fns.remap(next.handle, this.handle, Array.from(map)); } catch (e) { next.close(); throw e; }
    return next;
  };
  Class.prototype.snapshot = function snapshot(streams) {
    return fns.snapshot(this.handle, streams === undefined || streams === null ? null : Array.from(streams));
  };
  Class.fromSnapshot = function fromSnapshot(processor, buf, map, options = {}) {
    const info = xmodemSnapshotInfo(buf);
    if (XM_KINDS[info.kind] !== kind) throw new TypeError(`${Class.name}.fromSnapshot: the snapshot is of kind '${XM_KINDS[info.kind]}', not '${kind}'`);
    const m = map === undefined || map === null ? Array.from({ length: info.nStreams }, (_, i) => i) : Array.from(map);
    const next = made(processor, info, options);
    try { fns.restore(next.handle, buf, m); } catch (e) { next.close(); throw e; }
    return next;
  };
}
lifecycle(XModemReceiverBatch, 'rx', { remap: addon.xmodemRxRemap, snapshot: addon.xmodemRxSnapshot, restore: addon.xmodemRxRestore },
  (self, p) => new XModemReceiverBatch(p), (p) => new XModemReceiverBatch(p));
lifecycle(XModemSenderBatch, 'tx', { remap: addon.xmodemTxRemap, snapshot: addon.xmodemTxSnapshot, restore: addon.xmodemTxRestore },
  (self, p) => new XModemSenderBatch(p, { maxPayloadSize: self.maxPayloadSize, maxRetries: self.maxRetries }),
  (p, info, o) => new XModemSenderBatch(p, Object.assign({ maxPayloadSize: info.param0, maxRetries: info.param1 }, o)));
lifecycle(XModemFileReceiverBatch, 'recv', { remap: addon.xmodemRecvRemap, snapshot: addon.xmodemRecvSnapshot, restore: addon.xmodemRecvRestore },
  (self, p) => new XModemFileReceiverBatch(p, { fileCapacity: self.fileCapacity, maxRetries: self.maxRetries }),
  (p, info, o) => new XModemFileReceiverBatch(p, Object.assign({ fileCapacity: info.param0, maxRetries: info.param1 }, o)));

module.exports = { xmodemSnapshotInfo, xmodemTimerSnapshotInfo, XModemReceiverBatch, XModemSenderBatch, XModemFileReceiverBatch, XModemTimers, CRC16, XModemPacket, ControlType, PacketConstants, crc16Batch, serializeBatch, scanBursts };
