"""webaudio_modem_amd: MI355X-native batch FSK DSP engine behind the reference's FSKCore surface.

Everything that computes goes through libfskhip.so (hand-written HIP for gfx950, C ABI in
include/fskhip.h).  There is no CPU path in this package.
"""
from ._lib import FskHipError, PRECISION_F32, PRECISION_F64, DEMOD_WRITEBACK_AGC, LIB_PATH  # noqa: F401
from .engine import FSKEngine, DEFAULT_FSK_CONFIG, make_config, pinned_empty, snapshot_info, snapshot_stream_config, snapshot_concat, ingest_device, egress_device, SAMPLE_FORMATS, SAMPLE_LAYOUTS  # noqa: F401
from .fsk_core import FSKCore, Event, EventEmitter  # noqa: F401
from .filters import FilterDesign, FilterFactory, FIRFilter, FIRFilterBatch, IIRFilter, IIRFilterBatch, Upsampler, Downsampler, CaptureConverter, PlaybackConverter, resampler_snapshot_info, ratecvt_snapshot_info  # noqa: F401
from .processor import ChunkedModulator, FSKProcessorBatch, ProcessorBatchSnapshot, processor_snapshot_info, processor_snapshot_concat  # noqa: F401
from .xmodem import CRC16, XModemPacket, ControlType, crc16_batch, serialize_batch, scan_bursts, XModemReceiverBatch, XModemSenderBatch, XModemFileReceiverBatch, XModemTimers, xmodem_snapshot_info, xmodem_timer_snapshot_info  # noqa: F401
from . import sharding  # noqa: F401
from .sharded import FSKEngineSharded, FSKProcessorBatchSharded  # noqa: F401

__all__ = ["FSKEngine", "FSKEngineSharded", "FSKProcessorBatchSharded", "FSKCore", "FilterDesign", "FilterFactory", "FIRFilter", "FIRFilterBatch", "IIRFilter", "IIRFilterBatch", "Upsampler", "Downsampler", "CaptureConverter", "PlaybackConverter", "resampler_snapshot_info", "ratecvt_snapshot_info", "ChunkedModulator",
           "FSKProcessorBatch", "ProcessorBatchSnapshot", "processor_snapshot_info", "processor_snapshot_concat", "CRC16", "XModemPacket", "ControlType", "crc16_batch", "serialize_batch", "scan_bursts", "XModemReceiverBatch", "XModemSenderBatch", "XModemFileReceiverBatch", "XModemTimers", "xmodem_timer_snapshot_info",
           "DEFAULT_FSK_CONFIG", "snapshot_info", "snapshot_stream_config", "snapshot_concat", "ingest_device", "egress_device", "SAMPLE_FORMATS", "SAMPLE_LAYOUTS", "FskHipError", "PRECISION_F32", "PRECISION_F64"]
