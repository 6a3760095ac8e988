// Typings of napi/xmodem.js: CRC16 / XModemPacket / ControlType with the reference's surface (src/utils/crc16.ts,
// src/transports/xmodem/packet.ts, types.ts) plus the batch forms, the receive-grammar scan
// and the resident receiver over an FSKProcessorBatch's RX rings.
export declare const ControlType: Readonly<{ SOH: 0x01; ACK: 0x06; NAK: 0x15; EOT: 0x04 }>;
export declare const PacketConstants: Readonly<{ SOH: 0x01; HEADER_SIZE: 4; CRC_SIZE: 2; MIN_PACKET_SIZE: 6; MAX_PACKET_SIZE: 261;
  MAX_PAYLOAD_SIZE: 255; MAX_SEQUENCE: 255; MIN_DATA_SEQUENCE: 1 }>;
export interface DataPacket { soh: number; sequence: number; invSequence: number; length: number; payload: Uint8Array; checksum: number; }
export declare class CRC16 {
  static calculate(data: Uint8Array, device?: number): number;
  static verify(data: Uint8Array, expectedCrc: number, device?: number): boolean;
}
export declare class XModemPacket {
  static createData(sequence: number, payload: Uint8Array, device?: number): DataPacket;
  static serialize(packet: DataPacket): Uint8Array;
  static verify(packet: DataPacket, device?: number): boolean;
  static serializeControl(controlType: number): Uint8Array;
}
export declare function crc16Batch(rows: Uint8Array[], device?: number): Uint16Array;
export declare function serializeBatch(seqs: number[], payloads: Uint8Array[], device?: number): Uint8Array[];
export interface ScanResult {
  status: number; statusName: 'need_more' | 'eot' | 'truncated' | 'invalid_sequence' | 'invalid_crc' | 'unexpected_sequence';
  /** the reference's exception text where XModemTransport would throw (xmodem.ts:273, 290, 318), else null */
  error: string | null;
  expectedAfter: number; packets: number; dropped: number; consumed: number; errSeq: number; errLen: number; crcRx: number; crcCalc: number;
  data: Uint8Array;
}
export declare function scanBursts(bursts: Uint8Array[], expected: number | ArrayLike<number>, device?: number): ScanResult[];
export interface ReceiverState { expected: Uint32Array; packets: Uint32Array; dropped: Uint32Array; }
export interface PollResult {
  /** the streams with an event (an ACK or a NAK is owed), ascending */
  streams: Uint32Array;
  /** one per listed stream; `data` is that stream's accepted payload; statusName is never 'truncated': an incomplete packet waits */
  results: ScanResult[];
  /** CSR: the payload of streams[i] is data.subarray(offsets[i], offsets[i + 1]) */
  offsets: Uint32Array;
  data: Uint8Array;
}
/** XModemTransport's receive side for every stream of an FSKProcessorBatch (napi/fsk-processor.js), resident on the device. */
export declare class XModemReceiverBatch {
  constructor(processor: { handle: unknown; nStreams: number });
  readonly nStreams: number;
  poll(options?: { mask?: ArrayLike<boolean | number> | null }): PollResult;
  /** initializeReceive(): expectedSequence = 1 for one stream, or all (-1) */
  reset(stream?: number): void;
  state(): ReceiverState;
  setState(state: { expected?: ArrayLike<number> | null; packets?: ArrayLike<number> | null; dropped?: ArrayLike<number> | null }): void;
  close(): void;
  /** a new object over `processor` (the destination the engine and the processor were remapped into with the same map): stream i continues stream map[i], file included; -1 starts a new transport */
  remap(processor: object, map: ArrayLike<number>): XModemReceiverBatch;
  /** the image of `streams` (default: all, in order): words and files */
  snapshot(streams?: ArrayLike<number> | null): Buffer;
  /** a new object over `processor` continuing the records of a snapshot(); its parameters are the image's unless overridden */
  static fromSnapshot(processor: object, buf: Uint8Array, map?: ArrayLike<number> | null): XModemReceiverBatch;
}

/** fskhip_xmodem_tx_event of one stream */
export interface SenderEvent {
  status: number; statusName: 'progress' | 'done' | 'max_retries' | 'aborted';
  /** what sendData() would have thrown ('Operation aborted at sendData' where the abort ended the first wait), or null */
  error: string | null;
  stateAfter: number; stateName: string;
  /** the byte the wait returned (0x06 / 0x15 / 0x04), else -1 */
  control: number;
  /** bytes handed to the modulator by this poll: 0, 1 (EOT) or len + 6 */
  sentLen: number;
  sequence: number; fragmentIndex: number; nFragments: number; retries: number;
}
export interface SenderState {
  state: Uint32Array; sequence: Uint32Array; fragmentIndex: Uint32Array; retries: Uint32Array; packetsSent: Uint32Array; retransmitted: Uint32Array;
}
/** XModemTransport.sendData() for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_tx_*) */
export declare class XModemSenderBatch {
  constructor(processor: { handle: unknown; nStreams: number }, options?: { maxPayloadSize?: number; maxRetries?: number });
  readonly nStreams: number;
  readonly maxPayloadSize: number;
  readonly maxRetries: number;
  send(files: ArrayLike<ArrayLike<number> | null>, options?: { mask?: ArrayLike<boolean | number> | null }): void;
  /** one demodulate() reply per waiting stream; abort: the streams whose wait has timed out */
  poll(options?: { mask?: ArrayLike<boolean | number> | null; abort?: ArrayLike<boolean | number> | null }): { streams: Uint32Array; events: SenderEvent[] };
  /** reset(): IDLE, sequence 1, the file dropped, the counters 0, for one stream or all (-1) */
  reset(stream?: number): void;
  state(): SenderState;
  setState(state: { [K in keyof SenderState]?: ArrayLike<number> | null }): void;
  close(): void;
  /** a new object over `processor` (the destination the engine and the processor were remapped into with the same map): stream i continues stream map[i], file included; -1 starts a new transport */
  remap(processor: object, map: ArrayLike<number>): XModemSenderBatch;
  /** the image of `streams` (default: all, in order): words and files */
  snapshot(streams?: ArrayLike<number> | null): Buffer;
  /** a new object over `processor` continuing the records of a snapshot(); its parameters are the image's unless overridden */
  static fromSnapshot(processor: object, buf: Uint8Array, map?: ArrayLike<number> | null, options?: { maxRetries?: number }): XModemSenderBatch;
}

/** fskhip_xmodem_recv_event of one stream */
export interface FileReceiverEvent {
  status: number; statusName: 'progress' | 'done' | 'max_retries' | 'aborted' | 'file_full';
  /** what receiveData() would have thrown (the start of its text), or null */
  error: string | null;
  stateAfter: number; stateName: string;
  /** the byte transmitted by this poll (0x06 / 0x15), else -1 */
  control: number;
  /** the FSKHIP_XM_* status of the grammar step */
  step: number; stepName: string;
  /** of the packet concerned, else -1 */
  seq: number; len: number;
  /** bytes appended to the file by this poll */
  acceptedLen: number;
  fileLen: number; expected: number; retries: number; crcRx: number; crcCalc: number;
}
export interface FileReceiverState {
  state: Uint32Array; expected: Uint32Array; retries: Uint32Array; fileLen: Uint32Array; packetsReceived: Uint32Array; dropped: Uint32Array; packetsSent: Uint32Array;
}
/** XModemTransport.receiveData() for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_recv_*) */
export declare class XModemFileReceiverBatch {
  constructor(processor: { handle: unknown; nStreams: number }, options?: { fileCapacity?: number; maxRetries?: number });
  readonly nStreams: number;
  readonly fileCapacity: number;
  readonly maxRetries: number;
  /** receiveData() up to its first wait: the initial NAK is modulated */
  start(options?: { mask?: ArrayLike<boolean | number> | null }): void;
  /** at most one reply-owing step per waiting stream; timeout: the streams whose wait's timer has fired; abort: the streams to abort */
  poll(options?: { mask?: ArrayLike<boolean | number> | null; timeout?: ArrayLike<boolean | number> | null; abort?: ArrayLike<boolean | number> | null }):
    { streams: Uint32Array; events: FileReceiverEvent[] };
  /** the assembled files of `streams` (default: all) */
  files(streams?: ArrayLike<number> | null): Uint8Array[];
  setFiles(files: ArrayLike<ArrayLike<number> | null>, options?: { mask?: ArrayLike<boolean | number> | null }): void;
  /** reset(): IDLE, expected 1, retries 0, an empty file, the counters 0, for one stream or all (-1) */
  reset(stream?: number): void;
  state(): FileReceiverState;
  setState(state: { [K in keyof FileReceiverState]?: ArrayLike<number> | null }): void;
  close(): void;
  /** a new object over `processor` (the destination the engine and the processor were remapped into with the same map): stream i continues stream map[i], file included; -1 starts a new transport */
  remap(processor: object, map: ArrayLike<number>): XModemFileReceiverBatch;
  /** the image of `streams` (default: all, in order): words and files */
  snapshot(streams?: ArrayLike<number> | null): Buffer;
  /** a new object over `processor` continuing the records of a snapshot(); its parameters are the image's unless overridden */
  static fromSnapshot(processor: object, buf: Uint8Array, map?: ArrayLike<number> | null, options?: { fileCapacity?: number; maxRetries?: number }): XModemFileReceiverBatch;
}
export interface XModemSnapshotInfo { kind: 1 | 2 | 3; nStreams: number; param0: number; param1: number; fileBytes: number; }
/** what an XModem snapshot holds, after validating all of it on the host */
export declare function xmodemSnapshotInfo(buf: Uint8Array): XModemSnapshotInfo;

export interface XModemTimersState { waited: Uint32Array; mark: Uint32Array; }
/** the timeoutMs timers of sendData() / receiveData() for every stream of a file receiver or a sender, resident on the device in the
 * engine's sample clock (fskhip_xmodem_timer_*); quantised to the polls: poll once per quantum.  Close it before its handle. */
export declare class XModemTimers {
  /** timeoutSamples (default 144000: 3000 ms at 48 kHz), or timeoutMs with sampleRate (default 48000), rounded up */
  constructor(handle: XModemFileReceiverBatch | XModemSenderBatch, options?: { timeoutSamples?: number; timeoutMs?: number; sampleRate?: number });
  readonly nStreams: number;
  readonly timeoutSamples: number;
  /** the handle's own poll between a fire and an arm pass; elapsed: the engine samples processed since the previous poll; abort: the external abort */
  poll(elapsed: number, options?: { mask?: ArrayLike<boolean | number> | null; abort?: ArrayLike<boolean | number> | null }):
    { streams: Uint32Array; events: FileReceiverEvent[] | SenderEvent[] };
  /** waited 0, mark 0 for one stream or all (-1) */
  reset(stream?: number): void;
  /** waited: samples the current wait has lasted; mark: bits 0-1 the stage the timer was armed for, 4 was-pending */
  state(): XModemTimersState;
  setState(state: { [K in keyof XModemTimersState]?: ArrayLike<number> | null }): void;
  close(): void;
  /** a new object over `handle` (the receiver or sender this one's handle was remapped into with the same map): stream i continues the wait of stream map[i]; -1 is a fresh timer.  The timeout is this object's unless given */
  remap(handle: XModemFileReceiverBatch | XModemSenderBatch, map: ArrayLike<number>, options?: { timeoutSamples?: number }): XModemTimers;
  /** the image of `streams` (default: all, in order): two words per stream */
  snapshot(streams?: null | ArrayLike<number>): Buffer;
  /** a new object over `handle` continuing the records of a snapshot(); the timeout is the image's unless given.  TypeError where the image's kind is not the handle's */
  static fromSnapshot(handle: XModemFileReceiverBatch | XModemSenderBatch, buf: Uint8Array, map?: ArrayLike<number> | null, options?: { timeoutSamples?: number }): XModemTimers;
}
export interface XModemTimerSnapshotInfo { kind: 2 | 3; nStreams: number; timeoutSamples: number; }
/** what an XModemTimers snapshot holds, after validating all of it on the host */
export declare function xmodemTimerSnapshotInfo(buf: Uint8Array): XModemTimerSnapshotInfo;
