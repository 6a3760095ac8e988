// Typings of napi/filters.js: the FIR half of src/dsp/filters.ts.
export declare const PRECISION_F32: 0;
export declare const PRECISION_F64: 1;
export declare class FilterDesign {
  static sincLowpass(cutoffFreq: number, sampleRate: number, numTaps: number): number[];
  static sincHighpass(cutoffFreq: number, sampleRate: number, numTaps: number): number[];
  static sincBandpass(centerFreq: number, bandwidth: number, sampleRate: number, numTaps: number): number[];
}
export declare class FIRFilterBatch {
  constructor(coefficients: number[], nStreams?: number, options?: { device?: number; precision?: 0 | 1 });
  /** input: [nStreams][n] */
  processBuffer(input: Float32Array): Float32Array;
  reset(stream?: number): void;
  getCoefficients(): number[];
  close(): void;
}
export declare class FIRFilter extends FIRFilterBatch {
  constructor(coefficients: number[], options?: { device?: number; precision?: 0 | 1 });
  process(input: number): number;
}
export type SampleFormat = 'f32' | 's16' | 'mulaw' | 'alaw' | 0 | 1 | 2 | 3;
export type SampleLayout = 'stream' | 'sample' | 0 | 1;
export interface ResamplerOptions { taps?: number[]; lowRate?: number; device?: number; precision?: 0 | 1 }
/** Rate conversion by an integer factor on the GPU (fskhip_resampler_*); the history is carried across calls. */
declare class Resampler {
  readonly factor: number;
  readonly nStreams: number;
  readonly lowRate: number;
  readonly taps: number[];
  readonly history: number;
  reset(stream?: number): void;
  /** the history rows, [nStreams][history], oldest first */
  state(): Float32Array;
  setState(state: Float32Array): void;
  /** a new object of this design: stream i continues stream map[i] of this one, bit for bit (-1: a zero history) */
  remap(map: ArrayLike<number>): this;
  /** the image of `streams` (null: all, in order): the design and the history rows */
  snapshot(streams?: ArrayLike<number> | null): Buffer;
  close(): void;
}
export interface ResamplerSnapshotInfo { nStreams: number; direction: 0 | 1; factor: number; nTaps: number; precision: 0 | 1; history: number; taps: Float64Array }
/** what a resampler snapshot holds, validated on the host */
export declare function resamplerSnapshotInfo(buf: Uint8Array): ResamplerSnapshotInfo;
export declare class Upsampler extends Resampler {
  constructor(factor: number, nStreams: number, options?: ResamplerOptions);
  /** a new object from a snapshot() alone: stream i continues record map[i] (-1: a zero history; null: every record) */
  static fromSnapshot(buf: Uint8Array, map?: ArrayLike<number> | null, options?: { device?: number; lowRate?: number }): Upsampler;
  /** samples: [nStreams][pitch] or frames [nPerStream][pitch]; returns [nStreams][nPerStream * factor] */
  process(samples: Float32Array | Int16Array | Uint8Array, format: SampleFormat, layout?: SampleLayout, nPerStream?: number, pitch?: number): Float32Array;
}
export declare class Downsampler extends Resampler {
  constructor(factor: number, nStreams: number, options?: ResamplerOptions);
  static fromSnapshot(buf: Uint8Array, map?: ArrayLike<number> | null, options?: { device?: number; lowRate?: number }): Downsampler;
  /** input: [nStreams][n], n a multiple of factor; returns [nStreams][n / factor] or frames [n / factor][nStreams] */
  process(input: Float32Array, format: SampleFormat, layout?: SampleLayout, lens?: Uint32Array | null): Float32Array | Int16Array | Uint8Array;
}
export interface RateConverterOptions { taps?: number[]; device?: number; precision?: 0 | 1 }
/** Rate conversion by a ratio up / down on the GPU (fskhip_ratecvt_*): inRate -> outRate, the rates over their gcd; the history is carried across calls. */
declare class RateConverter {
  static ratio(inRate: number, outRate: number): { up: number; down: number };
  static defaultTaps(inRate: number, outRate: number): number[];
  readonly inRate: number;
  readonly outRate: number;
  readonly up: number;
  readonly down: number;
  readonly nStreams: number;
  readonly taps: number[];
  readonly history: number;
  /** samples per stream a call with nIn per stream (a multiple of down) gives */
  outCount(nIn: number): number;
  /** the inputs taken since the last period boundary, 0 .. down - 1, one number for all streams; 0 at creation and after reset() */
  readonly position: number;
  /** the by-hand carry of the position, beside state / setState */
  setPosition(pos: number): void;
  /** samples per stream processAny gives for nIn per stream (any) from the current position; possibly 0 */
  outCountAny(nIn: number): number;
  /** the fewest samples per stream for which processAny gives at least nOut from the current position */
  inCountAny(nOut: number): number;
  reset(stream?: number): void;
  /** the history rows, [nStreams][history], oldest first */
  state(): Float32Array;
  setState(state: Float32Array): void;
  /** a new object of this design, at this position, whose stream i continues stream map[i] of this one (-1: a zero history); the rows move on the device */
  remap(map: ArrayLike<number>): this;
  /** the image of `streams` (null: all, in order): the design, the position and the history rows */
  snapshot(streams?: ArrayLike<number> | null): Buffer;
  close(): void;
}
export interface RatecvtSnapshotInfo { nStreams: number; direction: 0 | 1; up: number; down: number; nTaps: number; precision: 0 | 1; history: number; position: number; taps: Float64Array }
/** where a restored converter lives, and its rates: an image knows up and down only (default: inRate = down, outRate = up) */
export interface RatecvtRestoreOptions { device?: number; inRate?: number; outRate?: number }
/** what a rate converter snapshot holds, validated on the host */
export declare function ratecvtSnapshotInfo(image: Uint8Array): RatecvtSnapshotInfo;
export declare class CaptureConverter extends RateConverter {
  constructor(inRate: number, outRate: number, nStreams: number, options?: RateConverterOptions);
  /** a new object from a snapshot() alone, at its position: stream i continues record map[i] (-1: a zero history; null: every record) */
  static fromSnapshot(image: Uint8Array, map?: ArrayLike<number> | null, device?: number | RatecvtRestoreOptions): CaptureConverter;
  /** samples: [nStreams][pitch] or frames [nIn][pitch], nIn a multiple of down; returns [nStreams][nIn / down * up] */
  process(samples: Float32Array | Int16Array | Uint8Array, format: SampleFormat, layout?: SampleLayout, nIn?: number, pitch?: number): Float32Array;
  /** process() for any nIn, from the handle's position; returns [nStreams][outCountAny(nIn)] and moves the position on */
  processAny(samples: Float32Array | Int16Array | Uint8Array, format: SampleFormat, layout?: SampleLayout, nIn?: number, pitch?: number): Float32Array;
}
export declare class PlaybackConverter extends RateConverter {
  constructor(inRate: number, outRate: number, nStreams: number, options?: RateConverterOptions);
  static fromSnapshot(image: Uint8Array, map?: ArrayLike<number> | null, device?: number | RatecvtRestoreOptions): PlaybackConverter;
  /** input: [nStreams][n], n a multiple of down; returns [nStreams][n / down * up] or frames [n / down * up][nStreams] */
  process(input: Float32Array, format: SampleFormat, layout?: SampleLayout, lens?: Uint32Array | null): Float32Array | Int16Array | Uint8Array;
  /** process() for any n, from the handle's position; returns [nStreams][outCountAny(n)] or frames and moves the position on */
  processAny(input: Float32Array, format: SampleFormat, layout?: SampleLayout, lens?: Uint32Array | null): Float32Array | Int16Array | Uint8Array;
  /** output samples that can be non-zero for a signal of n input samples */
  outLength(n: number): number;
}
export declare class FilterFactory {
  static createFIRLowpass(cutoffFreq: number, sampleRate: number, numTaps?: number): FIRFilter;
  static createFIRHighpass(cutoffFreq: number, sampleRate: number, numTaps?: number): FIRFilter;
  static createFIRBandpass(centerFreq: number, bandwidth: number, sampleRate: number, numTaps?: number): FIRFilter;
}
