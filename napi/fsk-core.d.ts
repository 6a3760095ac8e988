// Typings of napi/fsk-core.js: the reference's FSKConfig / IModulator surface (src/modems/fsk.ts:5-17,
// src/core.ts:88-117) plus the batch interface.
export interface FSKConfig {
  sampleRate: number; baudRate: number; markFrequency: number; spaceFrequency: number;
  preamblePattern: number[]; sfdPattern: number[]; startBits: number; stopBits: number;
  parity: 'none' | 'even' | 'odd'; syncThreshold: number; agcEnabled: boolean;
  preFilterBandwidth: number; adaptiveThreshold: boolean;
}
export const DEFAULT_FSK_CONFIG: FSKConfig;
export const PRECISION_F32: 0;
export const PRECISION_F64: 1;
export class Event { constructor(data?: unknown); readonly data: unknown; }
export class EventEmitter {
  on(eventName: string, callback: (event: Event) => void): void;
  off(eventName: string, callback: (event: Event) => void): void;
  emit(eventName: string, event?: Event): void;
  removeAllListeners(eventName?: string): void;
}
export interface FSKStatus {
  ready: boolean; frameStarted: boolean; globalSampleCounter: number; receivedBitsLength: number;
  byteBufferLength: number; demodulationCalls: number; syncDetections: number; silenceThreshold: number;
  totalSamplesProcessed: number; agcGain?: number; eodCount?: number;
}
export class FSKCore extends EventEmitter {
  constructor(options?: { device?: number; precision?: 0 | 1 });
  readonly name: 'FSK'; readonly type: 'FSK';
  configure(config: Partial<FSKConfig>): void;
  getConfig(): FSKConfig;
  modulateData(data: Uint8Array): Promise<Float32Array>;
  demodulateData(samples: Float32Array): Promise<Uint8Array>;
  reset(): void;
  isReady(): boolean;
  getSignalQuality(): { snr: number; ber: number; eyeOpening: number; phaseJitter: number; frequencyOffset: number };
  /** opt-in extension: real estimates (include/fskhip.h), off by default; getSignalQuality() keeps the reference's zeros */
  enableSignalQualityEstimates(on?: boolean): void;
  getSignalQualityEstimates(): SignalQualityEstimates;
  getStatus(): FSKStatus;
  close(): void;
}
export interface SignalQualityEstimates {
  snr: number; ber: number; eyeOpening: number; phaseJitter: number; frequencyOffset: number;
  signalLevel: number; noiseFloor: number; frames: number; bytes: number;
}
export type SampleArray = Int16Array | Uint8Array | Float32Array;
export type SampleFormat = 'f32' | 's16' | 'mulaw' | 'alaw' | 0 | 1 | 2 | 3;
export type SampleLayout = 'stream' | 'sample' | 0 | 1;
export const SAMPLE_FORMATS: { f32: 0; s16: 1; mulaw: 2; alaw: 3 };
export const SAMPLE_LAYOUTS: { stream: 0; sample: 1 };
export class FSKBatch {
  constructor(nStreams: number, configs: Partial<FSKConfig> | Partial<FSKConfig>[], options?: { device?: number; precision?: 0 | 1 });
  demodulateData(samples: Float32Array, nPerStream: number, pitch?: number, writebackAgc?: boolean): { bytes: Uint8Array[]; eod: Uint32Array };
  /** the same on a libuv worker thread (N-API async work); one call in flight per batch */
  demodulateDataAsync(samples: Float32Array, nPerStream: number, pitch?: number, writebackAgc?: boolean): Promise<{ bytes: Uint8Array[]; eod: Uint32Array }>;
  /** demodulateData for capture samples as they arrive: Int16Array ('s16'), G.711 Uint8Array ('mulaw' | 'alaw') or Float32Array ('f32'); layout 'stream' = [S][pitch], 'sample' = interleaved frames [nPerStream][pitch >= S] */
  demodulateSamples(samples: SampleArray, format: SampleFormat, layout: SampleLayout | undefined, nPerStream: number, pitch?: number): { bytes: Uint8Array[]; eod: Uint32Array };
  demodulateSamplesAsync(samples: SampleArray, format: SampleFormat, layout: SampleLayout | undefined, nPerStream: number, pitch?: number): Promise<{ bytes: Uint8Array[]; eod: Uint32Array }>;
  modulateData(payloads: Uint8Array[]): Float32Array[];
  /** modulateData into playback samples, quantised on the device: 's16' Int16Array, 'mulaw' | 'alaw' Uint8Array, 'f32' Float32Array; layout 'stream' = [S][pitch], 'sample' = interleaved frames [nPerStream][pitch >= S]; nPerStream undefined: the longest signal; stream s is the format's silence from lens[s] on */
  modulateSamples(payloads: Uint8Array[], format: SampleFormat, layout?: SampleLayout, nPerStream?: number, pitch?: number, out?: SampleArray): { samples: SampleArray; lens: Uint32Array; nPerStream: number; pitch: number };
  reset(stream?: number): void;
  getStatus(stream?: number): FSKStatus;
  /** 1 = the stream absorbed a NaN / Inf sample (dead from there on, like the reference's instance) or, fp32 engines, a sample beyond their range */
  getFaults(): Uint8Array;
  enableSignalQualityEstimates(on?: boolean): void;
  getSignalQualityEstimates(stream?: number): SignalQualityEstimates;
  /** a new batch of map.length streams: stream i continues stream map[i] of this one as if moved, or is new where map[i] is -1 */
  remap(map: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[]): FSKBatch;
  /** a portable image of streams `streams` (default: all, in order): plain bytes that a new batch on any device, in any process of the same build, continues from */
  snapshot(streams?: ArrayLike<number>): Buffer;
  /** a new batch whose stream i continues RECORD map[i] of the snapshot (-1: new; default: every record in order); precision and configs come from the snapshot unless given */
  static fromSnapshot(buf: Uint8Array, map?: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[], device?: number): FSKBatch;
  close(): void;
}
export interface SnapshotInfo {
  nStreams: number; precision: 0 | 1; perStreamConfigs: number; recordBytes: number; demodulationCalls: number; totalSamplesProcessed: number;
}
/** what a snapshot holds (validated on the host, no device needed) */
export function snapshotInfo(buf: Uint8Array): SnapshotInfo;
/** the records of several snapshots under one header; they must be images of engines that could have been one engine */
export function snapshotConcat(bufs: Uint8Array[]): Buffer;
/** one Node process, several GPUs: one FSKBatch per device over contiguous stream blocks, calls issued together */
export class FSKBatchSharded {
  constructor(nStreams: number, configs: Partial<FSKConfig> | Partial<FSKConfig>[], options?: { devices?: number[]; precision?: 0 | 1 });
  readonly shards: { first: number; count: number; device: number; batch: FSKBatch }[];
  demodulateData(samples: Float32Array, nPerStream: number, pitch?: number, writebackAgc?: boolean): Promise<{ bytes: Uint8Array[]; eod: Uint32Array }>;
  /** FSKBatch.demodulateSamples over the shards, no host copy: a shard takes a row block ('stream') or a column block with the full frame pitch ('sample') */
  demodulateSamples(samples: SampleArray, format: SampleFormat, layout: SampleLayout | undefined, nPerStream: number, pitch?: number): Promise<{ bytes: Uint8Array[]; eod: Uint32Array }>;
  modulateData(payloads: Uint8Array[]): Float32Array[];
  /** FSKBatch.modulateSamples over the shards into ONE array, no host copy: a shard writes a row block ('stream') or a column block at the full frame pitch ('sample') */
  modulateSamples(payloads: Uint8Array[], format: SampleFormat, layout?: SampleLayout, nPerStream?: number, pitch?: number, out?: SampleArray): { samples: SampleArray; lens: Uint32Array; nPerStream: number; pitch: number };
  reset(stream?: number): void;
  getStatus(stream?: number): FSKStatus;
  /** one snapshot of the whole batch, records in global stream order */
  snapshot(): Buffer;
  /** a new sharded batch whose stream i continues GLOBAL stream map[i] of this one (-1: new), across shards and devices (default: this batch's) */
  remap(map: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[], options?: { devices?: number[] }): FSKBatchSharded;
  close(): void;
}
