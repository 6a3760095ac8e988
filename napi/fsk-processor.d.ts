// Typings of napi/fsk-processor.js and napi/chunked-modulator.js (src/webaudio/processors/fsk-processor.ts,
// src/webaudio/chunked-modulator.ts on the device).
import { CaptureConverter, Downsampler, PlaybackConverter, Upsampler } from './filters';
import { FSKBatch, FSKConfig, FSKCore, FSKStatus, SampleArray, SampleFormat, SampleLayout } from './fsk-core';
export declare const PROC_CLEAR_RX_ON_TX_COMPLETE: 1;
export declare const PROC_GRAPH: 2;
/** a ratecvt quantum's TX side through the two launches its fused kernel replaces (measurements, tests) */
export declare const PROC_RATECVT_PAIR: 4;
/** FSKProcessorBatch.snapshot(): the FSKBatch's stream snapshot and the processors' own image */
export interface ProcessorBatchSnapshot { engine: Buffer; processor: Buffer; }
export declare function processorSnapshotInfo(buf: Uint8Array): { nStreams: number; rxCapacity: number; payloadCapacity: number; recordBytes: number };
/** fskhip_processor_snapshot_concat: the records of `bufs` in order under one header, canonical (host only). */
export declare function processorSnapshotConcat(bufs: Uint8Array[]): Buffer;
export declare class FSKProcessorBatch {
  constructor(batch: FSKBatch, options?: { rxCapacity?: number; clearRxOnTxComplete?: boolean; useGraph?: boolean });
  readonly nStreams: number;
  /** process(inputs, outputs) for every stream: inputs [S][nIn] or null; returns [S][nOut] or null */
  process(inputs: Float32Array | null, nIn: number, nOut: number): Float32Array | null;
  /** process() with either side in a capture format and layout: 'stream' = [S][pitch >= n], 'sample' = interleaved frames [n][pitch >= S];
   *  returns the output format's typed array (null when nOut is 0); state and output are process()'s on the decoded floats */
  processSamples(inputs: SampleArray | null, input?: { format?: SampleFormat; layout?: SampleLayout; nIn?: number; pitch?: number },
    output?: { format?: SampleFormat; layout?: SampleLayout; nOut?: number; pitch?: number }): SampleArray | null;
  /** processSamples() with both sides at the trunk's own rate, through an Upsampler / Downsampler of filters.js that carry their histories:
   *  nIn, nOut and the pitches count low rate elements; format defaults to 'mulaw', layout to 'sample'; a side without samples needs no handle.
   *  With a CaptureConverter / PlaybackConverter in the two slots both sides are at the converters' outer rate (44.1 kHz either side of a
   *  48 kHz engine): nIn is a multiple of the capture converter's `down`, nOut of the playback converter's `up`; one call takes resamplers
   *  or converters, not one of each */
  processSamplesAt(inputs: SampleArray | null,
    input?: { format?: SampleFormat; layout?: SampleLayout; nIn?: number; pitch?: number; upsampler?: Upsampler | CaptureConverter },
    output?: { format?: SampleFormat; layout?: SampleLayout; nOut?: number; pitch?: number; downsampler?: Downsampler | PlaybackConverter }): SampleArray | null;
  /** processSamplesAt() through a CaptureConverter and a PlaybackConverter for quanta of any length (128 frames at 44.1 kHz as they arrive):
   *  the handles carry their positions; state and samples are those of processAny -> process() -> processAny; a resampler is a TypeError */
  processSamplesAtAny(inputs: SampleArray | null,
    input?: { format?: SampleFormat; layout?: SampleLayout; nIn?: number; pitch?: number; upsampler?: CaptureConverter },
    output?: { format?: SampleFormat; layout?: SampleLayout; nOut?: number; pitch?: number; downsampler?: PlaybackConverter }): SampleArray | null;
  /** 'modulate': throws 'Modulation already in progress' when a selected stream still has one */
  modulate(payloads: Uint8Array[], mask?: boolean[]): void;
  /** the kernel that wrote the last quantum's output, or the two launches that stand for one joined by '+'
   *  ('processor_io_ratecvt_kernel<any>', 'processor_io_kernel+ratecvt_playback_any_kernel', ...); '' where it had no TX side */
  readonly lastTxKernel: string;
  txState(): { pos: Uint32Array; total: Uint32Array; pending: Uint8Array; completed: Uint32Array };
  /** 'demodulate' without the wait: everything buffered, per stream */
  demodulate(): Uint8Array[];
  /** the same for the streams that hold at least max(minLen, 1) bytes (and mask[s]) only, in ascending order: the bytes of
   *  streams[i] are data.subarray(offsets[i], offsets[i + 1]); streams not listed keep their rings */
  rxDrainSparse(options?: { mask?: ArrayLike<boolean | number> | null; minLen?: number }): { streams: Uint32Array; offsets: Uint32Array; data: Uint8Array };
  rxLengths(): Uint32Array;
  reset(stream?: number): void;
  status(stream?: number): FSKStatus & { demodulatedBufferLength: number; pendingModulation: boolean; fskCoreReady: boolean; processDemodulationCallCount: number };
  /** a new batch whose stream i continues stream map[i] of this one (FSKCore, ring, pending modulation), -1: a new stream */
  remap(map: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[]): FSKProcessorBatch;
  snapshot(streams?: ArrayLike<number>): ProcessorBatchSnapshot;
  static fromSnapshot(snap: ProcessorBatchSnapshot, map?: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[], device?: number,
    options?: { clearRxOnTxComplete?: boolean; useGraph?: boolean }): FSKProcessorBatch;
  close(): void;
}
export interface ShardedProcessorOptions { devices?: number[]; precision?: number; rxCapacity?: number; clearRxOnTxComplete?: boolean; useGraph?: boolean }
type ShardedInput<U> = { format?: SampleFormat; layout?: SampleLayout; nIn?: number; pitch?: number; upsampler?: U[] };
type ShardedOutput<D> = { format?: SampleFormat; layout?: SampleLayout; nOut?: number; pitch?: number; out?: SampleArray | null; downsampler?: D[] };
/** S FSKProcessors over several GPUs: one FSKBatch and one FSKProcessorBatch per device over contiguous blocks; FSKProcessorBatch's
 *  methods with global stream indices.  No host copy: a shard reads its row or column block of the caller's array and writes its block of
 *  ONE output (`out`, also accepted by FSKProcessorBatch's process forms).  The rate forms take arrays of handles, one per shard. */
export declare class FSKProcessorBatchSharded {
  constructor(nStreams: number, configs?: Partial<FSKConfig> | Partial<FSKConfig>[], options?: ShardedProcessorOptions);
  static blocks(nStreams: number, devices: number[]): { first: number; count: number; device: number }[];
  readonly nStreams: number;
  readonly shards: { first: number; count: number; device: number; batch: FSKBatch; procs: FSKProcessorBatch }[];
  readonly processors: FSKProcessorBatch[];
  readonly batches: FSKBatch[];
  processDemodulationCallCount: number;
  locate(stream: number): [{ first: number; count: number; device: number; batch: FSKBatch; procs: FSKProcessorBatch }, number];
  process(inputs: Float32Array | null, nIn: number, nOut: number, out?: Float32Array | null): Float32Array | null;
  processSamples(inputs: SampleArray | null, input?: ShardedInput<never>, output?: ShardedOutput<never>): SampleArray | null;
  processSamplesAt(inputs: SampleArray | null, input?: ShardedInput<Upsampler | CaptureConverter>, output?: ShardedOutput<Downsampler | PlaybackConverter>): SampleArray | null;
  processSamplesAtAny(inputs: SampleArray | null, input?: ShardedInput<CaptureConverter>, output?: ShardedOutput<PlaybackConverter>): SampleArray | null;
  /** one entry per shard */
  readonly lastTxKernel: string[];
  /** refuses the whole call, on every shard, when a selected stream still has a modulation pending */
  modulate(payloads: Uint8Array[], mask?: boolean[]): void;
  txState(): { pos: Uint32Array; total: Uint32Array; pending: Uint8Array; completed: Uint32Array };
  demodulate(): Uint8Array[];
  /** global stream numbers, ascending, and one CSR over all shards */
  rxDrainSparse(options?: { mask?: ArrayLike<boolean | number> | null; minLen?: number }): { streams: Uint32Array; offsets: Uint32Array; data: Uint8Array };
  rxLengths(): Uint32Array;
  reset(stream?: number): void;
  status(stream?: number): FSKStatus & { demodulatedBufferLength: number; pendingModulation: boolean; fskCoreReady: boolean; processDemodulationCallCount: number };
  /** stream i continues GLOBAL stream map[i] (-1: a new one) across shards and devices (options.devices: default this batch's) */
  remap(map: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[], options?: ShardedProcessorOptions): FSKProcessorBatchSharded;
  /** the shards' pairs under one header each (snapshotConcat, processorSnapshotConcat) */
  snapshot(): ProcessorBatchSnapshot;
  static fromSnapshot(snap: ProcessorBatchSnapshot, map?: ArrayLike<number>, configs?: Partial<FSKConfig> | Partial<FSKConfig>[],
    options?: ShardedProcessorOptions): FSKProcessorBatchSharded;
  close(): void;
}
export interface ChunkResult { signal: Float32Array; isComplete: boolean; samplesConsumed: number; totalSamples: number; }
export declare class ChunkedModulator {
  constructor(modulator: FSKCore);
  startModulation(data: Uint8Array): Promise<void>;
  getNextSamples(sampleCount: number): ChunkResult | null;
  isModulating(): boolean;
  getProgress(): number;
  cancel(): void;
  close(): void;
}
